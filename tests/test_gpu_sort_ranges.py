"""-m gpu: the depth sort (m2s_sort.hip) on crafted keys — every key-range branch at every size regime, against numpy.

After its key kernel the sort reads the smallest and the largest key back and takes one of three paths: `key - min` over the bits that
differ when they fit 24 ("reduced"), SubtractOrBehind over up to 32 bits when it applies the frustum test itself ("cull":
m2s_prepass_sorted without a depth image), else all 32 bits ("plain").  Under that the library chooses by n:
    rocPRIM of ROCm 7.2.0, rocprim/device/device_radix_sort.hpp: one block (256 threads x 4 items) for n <= 1024,
    merge sort up to radix_sort_config<>::merge_sort_limit = 1024 * 1024, onesweep above.
The inputs are tests/sort_cases.py's (test_sort_cases_cpu.py proves that they have the ranges their names say); the reference is
sort_cases.want_sorted / oracle.prepass + numpy's stable argsort on the depth bits — never a second device call.  Everything is compared
bit for bit.

ONE Converter serves the whole module, and every test walks its sizes down and up again: the grow-only buffers, the per-wave tables at
the work area's tail (placed from the buffer's capacity, not from n) and the position plane all meet a large n, then small ones, then a
large one."""
import ctypes

import numpy as np
import pytest

import camera
import sort_cases as sc
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.prepass import PrepassParams

pytestmark = pytest.mark.gpu

MERGE_SORT_LIMIT = 1024 * 1024          # see above
N_ONESWEEP = MERGE_SORT_LIMIT + 4097
VIEW, SECOND = sc.depth_view(), sc.second_view()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def assert_same_records(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        rows = np.flatnonzero((g != w).any(1))
        r = int(rows[0])
        raise AssertionError(f"{what}: {rows.size} of {g.shape[0]} sorted records differ, first at position {r}: key word {g[r, 0]:#010x} "
                             f"(record {g[r, sc.INDEX_WORD]}), expected {w[r, 0]:#010x} (record {w[r, sc.INDEX_WORD]})")


def sort_twice(conv, name, n):
    """upload -> sort (keys from the records; leaves the plane) -> sort by the second view (keys from the plane)"""
    rec = sc.records_with_keys(sc.key_bits(name, n), seed=n)
    conv.upload_records(rec)
    assert not conv.positions_ready
    assert_same_records(conv.sort_by_depth(VIEW), sc.want_sorted(rec, VIEW), f"{name}, n = {n}, first sort")
    assert conv.positions_ready
    assert_same_records(conv.sort_by_depth(SECOND), sc.want_sorted(rec, SECOND), f"{name}, n = {n}, second view, keys from the plane")


@pytest.mark.parametrize("name", sc.KEY_SETS)
def test_sort_by_depth_on_crafted_keys(conv, name):
    """range_0 .. range_ffffff: reduced (1 to 24 bits, on a denormal and on a large negative minimum); range_1000000, mixed_sign,
    denormals, quiet_nans: plain.  Sizes 1 .. 1024: one block; 1025 and 40 000: merge sort.  (quiet_nans: the device hands the two quiet
    NaNs through 1 * x + 0 with the bits numpy gives them, so they are compared like every other key.)"""
    for n in sc.down_and_up(sc.SIZES):
        sort_twice(conv, name, n)


def device_u32(hiplib, ptr, n):
    """uint32[n] at a device address: hipMemcpy of the HIP runtime the library itself is linked to (looked up through the library's
    handle: a process must not hold a second runtime)"""
    out = np.empty(n, np.uint32)
    assert hiplib.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(n * 4), 2) == 0      # device to host
    return out


def cull_params(**kw):
    """the camera at the origin looking down -z, no depth image: the sort applies the frustum test"""
    return PrepassParams(view_mat=np.eye(4, dtype=np.float32), proj_mat=camera.perspective(45.0, 1.0, 0.01, 100.0),
                         model_mat=np.eye(4, dtype=np.float32), renderer_resolution=(640, 640), resolution_target=48, **kw)


@pytest.mark.parametrize("n", [65, 1025, 40_000])
def test_sorted_keys_are_whole_once(conv, hiplib, n):
    """m2s_device_sorted_keys after a reduced sort (the keys on the device are key - min: the accessor puts min back, once), after a
    plain sort that follows it (nothing to put back: no offset may be left over), after a reduced sort from the plane, and after
    m2s_prepass_sorted (which reuses the key words: no sorted keys).  65: one block; 1025, 40 000: merge sort."""
    L, h = hiplib, conv._h

    def keys_twice(rec, view, what):
        assert conv.sort_by_depth(view, download=False) == n and L.m2s_num_sorted(h) == n
        want = np.sort(sc.want_keys(rec, view), kind="stable")
        for read in range(2):
            ptr = L.m2s_device_sorted_keys(h)
            assert ptr, what
            got = device_u32(L, ptr, n)
            assert np.array_equal(got, want), (what, f"read {read}", [hex(v) for v in got[:4]], [hex(v) for v in want[:4]])
        assert_same_records(conv.download_sorted(), sc.want_sorted(rec, view), what)

    reduced = sc.records_with_keys(sc.key_bits("range_ffffff_hi", n), seed=1)
    plain = sc.records_with_keys(sc.key_bits("range_1000000_hi", n), seed=2)
    assert int(sc.want_keys(reduced, VIEW).min()) == sc.MIN_HI           # (an offset that shows in every key)
    conv.upload_records(reduced)
    keys_twice(reduced, VIEW, "reduced")
    conv.upload_records(plain)
    keys_twice(plain, VIEW, "plain after reduced")
    conv.upload_records(reduced)
    keys_twice(reduced, VIEW, "reduced after plain")
    keys_twice(reduced, SECOND, "reduced, keys from the plane")
    mixed = sc.records_with_keys(sc.key_bits("mixed_sign", n), seed=3)
    conv.upload_records(mixed)
    keys_twice(mixed, SECOND, "plain (mixed signs) after reduced")
    # the sorted prepass shares the key words: the sort's keys are gone
    rec = sc.cull_records("cull_range_ffffff", n)
    conv.upload_records(rec)
    keys_twice(rec, sc.depth_view(axis=2), "reduced, before the sorted prepass")     # depth row (0, 0, 1, 0): the key is z itself
    assert conv.prepass_sorted(cull_params(), download=False) > 0
    assert L.m2s_device_sorted_keys(h) is None and L.m2s_num_sorted(h) == 0


def prepass_sorted_matches(conv, oracle, rec, p, n_alive, what):
    wk, wq, wd = oracle.prepass(p, rec)
    assert wk == n_alive and not np.isnan(wq).any(), (what, wk, n_alive)      # (the frustum test is the only one these records can fail)
    order = np.argsort(wd.view(np.uint32), kind="stable")
    want = wq[order]
    got = conv.prepass_sorted(p)
    assert got.shape == (wk, 24), (what, got.shape, wk)
    if not np.array_equal(bits(got), bits(want)):
        rows = np.flatnonzero((bits(got) != bits(want)).any(1))
        r = int(rows[0])
        raise AssertionError(f"{what}: {rows.size} of {wk} sorted quads differ, first at position {r}: from record {got[r, 19]:.0f}, "
                             f"expected record {want[r, 19]:.0f}")
    if wk:
        sources = np.flatnonzero(sc.frustum_test(rec, p.model_mat, p.view_mat, p.proj_mat)[0])[order]
        assert np.array_equal(want[:, 19], rec[sources, 20])   # (the reference's own record indices: q[4].w = pbr.x)
        assert np.array_equal(conv.download_sorted_sources(wk), sources.astype(np.uint32)), what
    else:
        assert not conv.device_sorted_sources, what


def prepass_frames(conv, oracle, name, n):
    """two frames of the same records (keys from the records, then from the plane), then one of the reversed records"""
    p = cull_params()
    rec = sc.cull_records(name, n)
    n_alive = int(sc.cull_survivors(name, n).sum())
    conv.upload_records(rec)
    for frame in range(2):
        prepass_sorted_matches(conv, oracle, rec, p, n_alive, f"{name}, n = {n}, frame {frame}")
    back = np.ascontiguousarray(rec[::-1])
    conv.upload_records(back)
    prepass_sorted_matches(conv, oracle, back, p, n_alive, f"{name}, n = {n}, reversed records")


@pytest.mark.parametrize("name", sc.CULL_SETS)
def test_prepass_sorted_on_crafted_depths(conv, oracle, name):
    """cull path throughout (no depth image), bit counts of `behind` = range + 1 from 1 to 27: cull_range_fffffe 24, cull_range_ffffff
    25 (none culled: cull_none), cull_wide / cull_whole_waves 27; one survivor (range 0, `behind` = 1); nothing survives (no sort at
    all).  Sizes 1 .. 65: one block; 1025, 40 000: merge sort."""
    for n in sc.down_and_up(sc.CULL_SIZES):
        prepass_frames(conv, oracle, name, n)


ONESWEEP_CASES = [("sort", "range_ffffff_hi", N_ONESWEEP), ("sort", "range_1000000_hi", N_ONESWEEP), ("sort", "mixed_sign", N_ONESWEEP),
                  ("prepass", "cull_range_ffffff", N_ONESWEEP), ("prepass", "cull_wide", N_ONESWEEP),
                  ("sort", "range_ffffff_hi", MERGE_SORT_LIMIT)]


@pytest.mark.parametrize("call,name,n", ONESWEEP_CASES)
def test_onesweep_regime(conv, oracle, call, name, n):
    """n = 2^20 + 4097, just past the merge sort's limit: onesweep — through the SubtractKey iterator over 24 bits (reduced:
    range_ffffff_hi), over all 32 bits (plain: range_1000000_hi, mixed_sign) and through the SubtractOrBehind iterator over 25 and 27 bits
    (cull: cull_range_ffffff, cull_wide).  n = 2^20 exactly: the last merge-sort size (reduced).  Each case twice: keys from the records,
    then from the plane."""
    if call == "sort":
        return sort_twice(conv, name, n)
    p = cull_params()
    rec = sc.cull_records(name, n)
    conv.upload_records(rec)
    wk, wq, wd = oracle.prepass(p, rec)
    alive = sc.cull_survivors(name, n)
    assert wk == int(alive.sum()) and not np.isnan(wq).any()
    order = np.argsort(wd.view(np.uint32), kind="stable")
    want = wq[order]
    sources = np.flatnonzero(alive)[order].astype(np.uint32)
    for frame in range(2):
        got = conv.prepass_sorted(p)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (name, frame)
        assert np.array_equal(conv.download_sorted_sources(wk), sources), (name, frame)
