"""-m gpu: m2s_merge with m2s_set_carry_sh on (Converter.carry_sh, .upload_sh, .sh_plane_info) against the numpy restatement of pin 5s
(tests/merge_sh_ref.py).  Records and map are what the merge without the switch gives, byte for byte; a singleton's row of the plane is
a copy and every other coefficient lies within 1 fp32 ulp of max_i |sh_ik| of the restatement's (the derivation: merge_sh_ref's
docstring).  Then what the switch leaves alone (off, no plane, a dry run, adopted memory), what follows a merged plane (export, prune, a
second merge), the errors of m2s_upload_sh, and 300 003 records."""
import ctypes as C
import os

import numpy as np
import pytest

import compact_ref as cr
import merge_ref as mr
import merge_sh_ref as ms
from mesh2splat_amd import synth
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams

pytestmark = pytest.mark.gpu
F = np.float32
CONFIGS = ((10, 4, 0.5, False), (3, 5, 0.5, False), (10, 64, -2.0, False), (10, 4, 0.5, True))
WORST = {"ulps": 0.0}                                                # over the module: printed by the last test


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain(hiplib):
    c = Converter(0)                                                 # never has the switch on
    yield c
    c.close()


def check(conv, plain, rec, sh, level, max_group, dot, unsigned=False, upload=True):
    """merge() with the switch on against the restatement and against the merge without it -> (records, map, plane) after"""
    want, wmap, wcounts, info, wplane, pinfo = ms.merge(rec, sh, level, max_group, dot, unsigned)
    if upload:
        conv.upload_records(rec)
        conv.upload_sh(sh)
    assert conv.sh_plane_info() == {"rows": len(rec), "degree": 3}
    conv.carry_sh = True
    got_counts = conv.merge(level, max_group, dot, unsigned_axis=unsigned)
    assert got_counts == wcounts == conv.last_merge_counts(), (got_counts, wcounts)
    gmap, got = conv.download_merge_map(), conv.download()
    assert np.array_equal(gmap, wmap)
    err = mr.compare(got, want, info)
    assert err["scalar_ulps"] <= mr.SCALAR_ULPS_BAR and err["cov_rel"] <= mr.COV_REL_BAR, err
    plain.upload_records(rec)
    assert plain.merge(level, max_group, dot, unsigned_axis=unsigned) == wcounts
    assert np.array_equal(bits(got), bits(plain.download())) and np.array_equal(gmap, plain.download_merge_map())   # the switch moves no record
    assert plain.device_sh == 0 and plain.last_merge_sh_ms == 0.0
    assert conv.sh_plane_info() == {"rows": wcounts["after"], "degree": 3} and conv.device_sh
    plane = conv.download_sh()
    assert plane.shape == wplane.shape
    ulps = ms.compare(plane, wplane, pinfo)
    print(f"merge+sh n={len(rec)} level={level} group={max_group} dot={dot} unsigned={unsigned}: {wcounts}, "
          f"unit {int(pinfo['unit'].sum())} by_area {int(pinfo['by_area'].sum())}, plane {ulps:.4f} ulp of max|sh|, sh {conv.last_merge_sh_ms:.3f} ms")
    WORST["ulps"] = max(WORST["ulps"], ulps)
    assert ulps <= ms.PLANE_ULPS_BAR
    return got, gmap, plane


@pytest.mark.parametrize("nonfinite", (False, True))
@pytest.mark.parametrize("level,max_group,dot,unsigned", CONFIGS)
def test_plane_against_the_restatement(conv, plain, level, max_group, dot, unsigned, nonfinite):
    rec = mr.crafted_records(300, 11)
    sh = ms.random_plane(300, 11, nonfinite, cr.valid_mask(rec))
    _, _, plane = check(conv, plain, rec, sh, level, max_group, dot, unsigned)
    assert conv.last_merge_counts()["merged"] > 0
    if nonfinite:
        assert np.isnan(plane).any() and np.isinf(plane).any()
    else:
        assert np.isfinite(plane).all()
    again = check(conv, plain, rec, sh, level, max_group, dot, unsigned)             # two runs give the same bytes
    assert np.array_equal(bits(plane), bits(again[2]))


def test_switch_off_or_no_plane_or_a_dry_run(conv, plain):
    rec = mr.crafted_records(300, 11)
    sh = ms.random_plane(300, 11)
    plain.upload_records(rec)
    plain.merge(3, 4, 0.5)
    want, wmap = plain.download(), plain.download_merge_map()
    # off: the plane is dropped as it always was
    conv.carry_sh = False
    assert not conv.carry_sh
    conv.upload_records(rec)
    conv.upload_sh(sh)
    assert conv.device_sh
    conv.merge(3, 4, 0.5)
    assert conv.device_sh == 0 and conv.last_merge_sh_ms == 0.0
    with pytest.raises(M2SError):
        conv.sh_plane_info()
    assert np.array_equal(bits(conv.download()), bits(want))
    # on without a plane: the same
    conv.carry_sh = True
    assert conv.carry_sh
    conv.upload_records(rec)
    conv.merge(3, 4, 0.5)
    assert conv.device_sh == 0 and conv.last_merge_sh_ms == 0.0 and np.array_equal(bits(conv.download()), bits(want))
    assert np.array_equal(conv.download_merge_map(), wmap)
    # on with a plane of OTHER records (a stale tag): dropped too
    conv.upload_records(rec)
    conv.upload_sh(sh)
    conv.upload_records(rec)
    conv.merge(3, 4, 0.5)
    assert conv.device_sh == 0 and np.array_equal(bits(conv.download()), bits(want))
    # a dry run changes nothing
    conv.upload_records(rec)
    conv.upload_sh(sh, degree=2)
    ptr = conv.device_records
    dry = conv.merge(3, 4, 0.5, dry_run=True)
    assert dry["after"] == len(want) and conv.device_records == ptr and conv.num_stored == 300 and conv.last_merge_sh_ms == 0.0
    assert conv.sh_plane_info() == {"rows": 300, "degree": 2} and np.array_equal(bits(conv.download_sh()), bits(sh))
    conv.merge(3, 4, 0.5)
    assert conv.sh_plane_info() == {"rows": len(want), "degree": 2}                    # the degree is kept


def test_adopted_memory_is_not_written(conv, plain):
    rec = mr.crafted_records(1000, 13)
    sh = ms.random_plane(1000, 13)
    owner = Converter(0)
    try:
        owner.upload_records(rec)
        conv.set_records(owner.device_records, len(rec), 64)
        conv.upload_sh(sh)
        check(conv, plain, rec, sh, 3, 5, 0.5, upload=False)
        assert conv.device_records != owner.device_records
        assert np.array_equal(bits(owner.download()), bits(rec))
    finally:
        owner.close()


def test_bake_merge_export_and_prune(conv, tmp_path):
    conv.carry_sh = True
    conv.upload_scene(synth.unit_quad())
    R = 16
    n = conv.convert(R)
    baked = conv.bake_light(BakeParams(n_theta=4, n_phi=8, use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)))
    assert baked.shape == (n, 48) and np.array_equal(bits(conv.download_sh()), bits(baked))   # download_sh after a bake: unchanged
    rec = conv.download()
    counts = conv.merge(8, 4, 0.5, unsigned_axis=True)                                # (a quarter of the box per cell: 4 x 4 records of R = 16)
    assert counts["merged"] > 0 and counts["after"] < n
    m = counts["after"]
    after, plane = conv.download(), conv.download_sh()
    perm, heads = ms.heads_of(rec, 8, 4, 0.5, True)
    wplane, pinfo = ms.merge_plane(rec, baked, perm, heads)
    assert ms.compare(plane, wplane, pinfo) <= ms.PLANE_ULPS_BAR
    py, host = str(tmp_path / "merged.ply"), str(tmp_path / "host.ply")
    conv.export_ply_sh(py, 0.65)
    assert conv._L.m2s_write_ply_sh(os.fsencode(host), after.ctypes.data, plane.ctypes.data, m, C.c_float(np.float32(0.65) / np.float32(R))) == 0
    assert open(py, "rb").read() == open(host, "rb").read()
    # a prune after the merge compacts the merged plane
    conv.contrib_begin()
    conv.upload_contrib(np.full(m, 0.5, F), np.arange(m, dtype=np.uint32))
    kept = conv.prune(0.0, m // 2)
    assert kept["kept"] == m - m // 2 and conv.sh_plane_info()["rows"] == kept["kept"]
    assert np.array_equal(bits(conv.download_sh()), bits(plane[m // 2:])) and np.array_equal(bits(conv.download()), bits(after[m // 2:]))


def test_upload_sh_errors(hiplib):
    c = Converter(0)
    try:
        sh = np.zeros((20, 48), F)
        rows, degree = C.c_uint64(), C.c_uint32()
        assert hiplib.m2s_upload_sh(c._h, sh.ctypes.data, 20, 3) == 7                # no records
        assert hiplib.m2s_sh_plane_info(c._h, C.byref(rows), C.byref(degree)) == 7
        c.upload_records(mr.crafted_records(20, 1))
        assert hiplib.m2s_upload_sh(c._h, sh.ctypes.data, 19, 3) == 1 and hiplib.m2s_upload_sh(c._h, sh.ctypes.data, 21, 3) == 1
        assert hiplib.m2s_upload_sh(c._h, sh.ctypes.data, 20, 4) == 1 and hiplib.m2s_upload_sh(c._h, None, 20, 3) == 1
        assert hiplib.m2s_sh_plane_info(c._h, C.byref(rows), C.byref(degree)) == 7 and c.device_sh == 0
        assert hiplib.m2s_upload_sh(c._h, sh.ctypes.data, 20, 1) == 0
        assert hiplib.m2s_sh_plane_info(c._h, C.byref(rows), C.byref(degree)) == 0 and (rows.value, degree.value) == (20, 1)
        assert hiplib.m2s_sh_plane_info(c._h, None, None) == 0
        c.upload_records(np.zeros((0, 24), F))                                       # no rows: a NULL plane is fine
        assert hiplib.m2s_upload_sh(c._h, None, 0, 3) == 0 and c.sh_plane_info() == {"rows": 0, "degree": 3} and c.download_sh().shape == (0, 48)
        # conversions in flight, then stale records
        c.upload_scene(synth.cube_sphere(6, tex_size=16))
        c.submit(48)
        total = c.wait()
        big = np.zeros((total, 48), F)
        c.submit(48)
        assert hiplib.m2s_upload_sh(c._h, big.ctypes.data, total, 3) == 7 and b"in flight" in hiplib.m2s_last_error(c._h)
        assert c.wait() == total
        assert hiplib.m2s_upload_sh(c._h, big.ctypes.data, total, 3) == 0
    finally:
        c.close()


def test_more_than_one_trip_and_a_second_merge_on_the_first(conv, plain):
    """300 003 records: some 4 700 segments of 64 members and the invalid singletons behind them — 221 workgroups of the reduction, a
    partial last wave — then at group 4 some 75 000 segments; the second merge runs on the first's result, whose plane lives in the
    buffer the first one wrote."""
    n = 300003
    rng = np.random.default_rng(5)
    base = mr.crafted_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    sh = ms.random_plane(n, 5)
    perm, heads = ms.heads_of(rec, 10, 4, -2.0)
    wplane, pinfo = ms.merge_plane(rec, sh, perm, heads)
    conv.carry_sh = True
    conv.upload_records(rec)
    conv.upload_sh(sh)
    counts = conv.merge(10, 4, -2.0)
    assert counts["after"] == len(heads) > 70000
    first_rec, first_plane = conv.download(), conv.download_sh()
    ulps = ms.compare(first_plane, wplane, pinfo)
    perm2, heads2 = ms.heads_of(first_rec, 10, 64, -2.0)
    wplane2, pinfo2 = ms.merge_plane(first_rec, first_plane, perm2, heads2)
    assert conv.merge(10, 64, -2.0)["after"] == len(heads2) and int(pinfo2["members"].max()) == 64
    ulps2 = ms.compare(conv.download_sh(), wplane2, pinfo2)
    print(f"merge+sh n={n}: {len(heads)} then {len(heads2)} segments, plane {ulps:.4f} / {ulps2:.4f} ulp of max|sh|, sh {conv.last_merge_sh_ms:.3f} ms")
    WORST["ulps"] = max(WORST["ulps"], ulps, ulps2)
    assert ulps <= ms.PLANE_ULPS_BAR and ulps2 <= ms.PLANE_ULPS_BAR
    assert conv.sh_plane_info()["rows"] == len(heads2) == conv.num_stored


def test_zz_worst_ratio_over_the_module():
    """Runs last in this module: the largest |got - want| of a merged coefficient in fp32 ulps of max_i |sh_ik| (the bar is 1)."""
    print(f"merge+sh, achieved over the module: {WORST['ulps']:.4f} ulp of max|sh| (bar {ms.PLANE_ULPS_BAR})")
    assert WORST["ulps"] <= ms.PLANE_ULPS_BAR
