"""Conditions on the fixtures of tests/test_gpu_prepass_sorted_lastcull.py, on the CPU oracle alone: prepass_cases.needle_records must
hold records that pass the frustum test and fail the shader's LAST test (lambda2 < 0, gaussianSplattingPrepassCS.glsl:183) at every
camera those tests use — the records on which m2s_prepass_sorted's dense path has to give way to the compacting one — and the ordinary
and hostile records must hold none (which is why the older tests never reached that branch).  A GPU test cannot then pass because its
input went soft."""
import numpy as np
import pytest

import prepass_cases as pcs

CASES = dict(pcs.cases())


@pytest.fixture(scope="module")
def needles():
    return pcs.needle_records(2000)


@pytest.mark.parametrize("name", ["colour", "model_trs", "ply_classic"])
@pytest.mark.parametrize("frame", [0, 1])
def test_needles_fail_the_last_test_by_the_hundred(oracle, needles, name, frame):
    p = CASES[name] if frame == 0 else pcs.second_frame(CASES[name])
    culls = pcs.last_test_culls(oracle, p, needles)
    print(f"{name}, frame {frame}: {culls.size} of {needles.shape[0]} needles fail the last test alone")
    assert culls.size >= 100


def test_needles_fail_the_last_test_with_the_camera_inside(oracle, needles):
    culls = pcs.last_test_culls(oracle, CASES["inside"], needles)
    print(f"inside: {culls.size} needles fail the last test alone")
    assert culls.size >= 10


def test_needles_fail_the_last_test_in_every_orbit_view(oracle, needles):
    views = pcs.orbit_views(64)
    assert len(views) == 6
    counts = [pcs.last_test_culls(oracle, p, needles).size for p in views]
    print(f"orbit views: {counts}")
    assert min(counts) >= 20


def test_last_test_culls_are_the_difference_of_two_prepasses(oracle, needles):
    """The helper itself: its indices are in frustum (the same records as small spheres survive), are missing from the oracle's prepass
    of the records as they are, and every other in-frustum record is in it."""
    p = CASES["colour"]
    culls = pcs.last_test_culls(oracle, p, needles)
    kept = pcs.surviving_records(oracle, p, needles)
    assert np.intersect1d(culls, kept).size == 0
    assert oracle.prepass(p, needles[culls])[0] == 0
    rest = np.setdiff1d(np.arange(needles.shape[0]), culls)
    assert oracle.prepass(p, needles[rest])[0] == kept.size == oracle.prepass(p, needles)[0]


def test_ordinary_and_hostile_records_never_fail_it(oracle):
    base = pcs.base_records(oracle, 14, 64)
    for rec, what in ((base, "base"), (pcs.hostile_records(2048), "hostile 2048"), (pcs.hostile_records(4096), "hostile 4096")):
        for name in ("colour", "model_trs", "ply_classic", "inside"):
            for p in (CASES[name], pcs.second_frame(CASES[name])):
                assert pcs.last_test_culls(oracle, p, rec).size == 0, (what, name)
    for p in pcs.orbit_views(64):
        assert pcs.last_test_culls(oracle, p, base).size == 0


def test_mixed_records_keep_the_needles_in_the_middle(oracle, needles):
    rec = pcs.mixed_records(oracle)
    n_front = pcs.base_records(oracle, 14, 64).shape[0] + 2048
    assert rec.shape[0] == n_front + 2000 + 3000 < 20000
    assert np.array_equal(rec[n_front:n_front + 2000].view(np.uint32), needles.view(np.uint32))
    assert np.array_equal(rec[-3000:].view(np.uint32), rec[:3000].view(np.uint32))
    culls = pcs.last_test_culls(oracle, CASES["colour"], rec)
    assert culls.size >= 100 and culls.min() >= n_front and culls.max() < n_front + 2000
