"""-m gpu: `mesh2splat in.glb out.ply --budget N`: the JSON record and the rows of the .ply, with and without --prune, the usage
errors, and the reason the option exists: a cap cuts the last mesh off, a budget does not."""
import json
import os
import subprocess

import numpy as np
import pytest

from mesh2splat_amd import _lib, gltf_io, synth

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
R, N = 32, 400
FIELDS = {"importance", "max_records", "before", "candidates", "kept", "threshold_key", "ties_kept", "ties", "cap_lifted"}


@pytest.fixture(scope="module")
def glb(tmp_path_factory, hiplib):
    """two spheres of 192 triangles side by side: mesh 0 round x = 0, mesh 1 round x = 2.5"""
    path = str(tmp_path_factory.mktemp("budget") / "two.glb")
    gltf_io.write_glb(synth.sphere_row(2, n=4, tex_size=16), path)
    return path


def run(glb, out, *args):
    r = subprocess.run([EXE, glb, out, "--density", str(R), "--format", "1", "--preview-size", "96x64", *args], capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("budget: ")]
    return r, [json.loads(ln[len("budget: "):]) for ln in lines]


def in_last_mesh(path):
    rec, _ = gltf_io.read_ply(path)
    return rec.shape[0], int((rec[:, 0] > 1.25).sum())          # (mesh 0 ends at x = 1, mesh 1 starts at x = 1.5)


def test_cli_budget_area_against_cap(glb, tmp_path):
    out = str(tmp_path / "b.ply")
    r, js = run(glb, out, "--budget", str(N))
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    j = js[0]
    assert set(j) == FIELDS and j["importance"] == "area" and j["max_records"] == N and j["cap_lifted"] is True
    assert j["before"] == j["candidates"] > N == j["kept"] and 1 <= j["ties_kept"] <= j["ties"] and j["threshold_key"] > 0
    rows, last = in_last_mesh(out)
    assert rows == N and last > 0 and f"({N} stored)" in r.stdout
    # the same count through the cap: the canonical order decides, and the last mesh is gone
    capped = str(tmp_path / "c.ply")
    r2, js2 = run(glb, capped, "--cap", str(N))
    assert r2.returncode == 0 and not js2, r2.stdout + r2.stderr
    assert in_last_mesh(capped) == (N, 0)
    # an explicit cap is honoured: the budget then chooses among what the cap left
    r3, js3 = run(glb, out, "--budget", str(N // 2), "--cap", str(N))
    assert r3.returncode == 0 and js3[0]["cap_lifted"] is False and js3[0]["before"] == N and js3[0]["kept"] == N // 2
    assert in_last_mesh(out) == (N // 2, 0)


def test_cli_budget_views(glb, tmp_path):
    out = str(tmp_path / "v.ply")
    r, js = run(glb, out, "--prune", "4", "--budget", str(N))
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    j = js[0]
    assert j["importance"] == "views" and j["kept"] == min(N, j["candidates"]) and j["candidates"] <= j["before"]
    prune = [json.loads(ln[len("prune: "):]) for ln in r.stdout.splitlines() if ln.startswith("prune: ")]
    assert len(prune) == 1 and prune[0]["kept"] == j["kept"] and prune[0]["before"] == j["before"] and len(prune[0]["eyes"]) == 12
    assert prune[0]["dropped_thresholds"] == j["before"] - j["candidates"] and prune[0]["dropped_budget"] == j["candidates"] - j["kept"]
    assert in_last_mesh(out)[0] == j["kept"]


def test_cli_budget_batch(glb, tmp_path):
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(out_dir), "--density", str(R), "--format", "1", "--budget", str(N)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = [json.loads(ln[len("budget: "):]) for ln in r.stdout.splitlines() if ln.startswith("budget: ")]
    assert len(js) == 1 and js[0]["kept"] == N and js[0]["importance"] == "area"
    assert in_last_mesh(str(out_dir / "two.ply"))[0] == N
    report = [ln for ln in r.stdout.splitlines() if "two.glb ->" in ln]
    assert len(report) == 1 and " ms, budget " in report[0]                     # the selection is timed apart from the conversion


def test_cli_budget_usage_errors(glb, tmp_path):
    out = str(tmp_path / "e.ply")
    for bad in (["--budget", str(N), "--gpus", "2"], ["--budget", "0"], ["--budget", "-3"], ["--budget"]):
        r, _ = run(glb, out, *bad)
        assert r.returncode == 2 and "usage:" in r.stderr, (bad, r.returncode, r.stderr[:200])
