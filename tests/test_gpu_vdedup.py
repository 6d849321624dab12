"""-m gpu: the vertex deduplication of mesh2splat_amd/csrc/m2s_vdedup.hip against a host std::map, on the GPU the suite runs on.

tests/vdedup/vdedup_check.hip links that translation unit and runs, once, every case listed in its main(): the caller's cube_sphere(4),
a soup without sharing, 200 triangles of one vertex, rows that differ in the sign of a zero or a NaN's payload, one triangle, corner
counts on both sides of a hash-table size, and both "not eligible" exits with small limits.  Per case: table[id[c]] == corner c
bitwise, the row count is the map's, ids are ranks in first-occurrence order, two runs agree."""
import json
import os
import subprocess

import pytest

from mesh2splat_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "vdedup", "_build", "vdedup_check")

CASES = ("file", "grid_8", "soup_300_no_sharing", "one_vertex_200_triangles", "signed_zero_and_nan_payload", "one_triangle",
         "hash_boundary_below", "hash_boundary_above", "id_limit_reached", "id_limit_not_reached", "sharing_too_low", "sharing_just_enough")


def test_dedup_against_a_host_map(tmp_path):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.dirname(os.path.dirname(EXE))], check=True, stdout=subprocess.DEVNULL)
    v = synth.cube_sphere_vertices(4)
    assert v.shape == (6 * 4 * 4 * 2 * 3, 12)
    path = tmp_path / "cube_sphere4.f32"
    v.astype("<f4").tofile(path)
    r = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=120)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    by = {ln["case"]: ln for ln in lines if "case" in ln}
    assert set(by) == set(CASES), sorted(by)
    for name, ln in by.items():
        assert ln["ok"] and ln["rows"] == ln["rows_ref"] and ln["bad_rows"] == 0 and ln["ids_out_of_order"] == 0 and ln["runs_equal"], ln
    assert by["file"]["eligible"] and by["file"]["triangles"] == 192 and by["file"]["rows"] < 192 * 3 // 2
    assert by["soup_300_no_sharing"]["rows"] == 900 and not by["soup_300_no_sharing"]["eligible"]
    assert by["one_vertex_200_triangles"]["rows"] == 1
    assert by["signed_zero_and_nan_payload"]["rows"] == 4
    assert by["one_triangle"]["rows"] == 3
    assert by["hash_boundary_below"]["hash_words"] * 2 == by["hash_boundary_above"]["hash_words"]
    assert not by["id_limit_reached"]["eligible"] and by["id_limit_not_reached"]["eligible"]
    assert not by["sharing_too_low"]["eligible"] and by["sharing_just_enough"]["eligible"]
    assert lines[-1] == {"all_ok": True}
