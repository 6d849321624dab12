"""-m gpu: `mesh2splat in.glb out.ply --merge-level L | --merge-to N`: the JSON record and the rows of the .ply, --merge-to followed by
--refit, --batch, and the usage errors."""
import json
import os
import subprocess

import pytest

from mesh2splat_amd import _lib, gltf_io, synth

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
R = 32
FIELDS = {"level", "max_group", "min_axis_dot", "target", "met", "before", "after", "merged", "invalid", "stage_ms"}


@pytest.fixture(scope="module")
def glb(tmp_path_factory, hiplib):
    path = str(tmp_path_factory.mktemp("merge") / "two.glb")
    gltf_io.write_glb(synth.sphere_row(2, n=4, tex_size=16), path)
    return path


def run(glb, out, *args):
    r = subprocess.run([EXE, glb, out, "--density", str(R), "--format", "1", "--preview-size", "96x64", *args], capture_output=True, text=True, timeout=300)
    return r, [json.loads(ln[len("merge: "):]) for ln in r.stdout.splitlines() if ln.startswith("merge: ")]


def rows(path):
    return gltf_io.read_ply(path)[0].shape[0]


def test_cli_merge_level_and_merge_to(glb, tmp_path):
    out = str(tmp_path / "m.ply")
    r, js = run(glb, out, "--merge-level", "6", "--merge-group", "8", "--merge-dot", "0.25")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    j = js[0]
    assert set(j) == FIELDS and (j["level"], j["max_group"], j["min_axis_dot"], j["target"], j["met"]) == (6, 8, 0.25, None, True)
    assert j["before"] > j["after"] == rows(out) and 0 < j["merged"] <= j["after"] and j["invalid"] == 0 and len(j["stage_ms"]) == 3
    n = j["before"]
    # --merge-to: the finest level that fits, which the level below does not (the spheres are coarse: half their edges break a run at
    # the default 0.5, so two thirds of the records is a target the defaults can meet and a fifth is not)
    N = 2 * n // 3
    r, js = run(glb, out, "--merge-to", str(N))
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    j = js[0]
    assert j["target"] == N and j["met"] is True and j["before"] == n and j["after"] == rows(out) <= N and j["max_group"] == 4
    if j["level"] > 0:
        r2, js2 = run(glb, out, "--merge-level", str(j["level"] - 1))
        assert r2.returncode == 0 and js2[0]["after"] > N
    r, js = run(glb, out, "--merge-to", str(n // 5))
    assert r.returncode == 0 and js[0]["met"] is False and js[0]["level"] == 10 and js[0]["after"] == rows(out) > n // 5


def test_cli_merge_to_then_refit(glb, tmp_path):
    out = str(tmp_path / "r.ply")
    r, js = run(glb, out, "--merge-to", "2600", "--refit", "1", "--refit-iters", "1")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    refit = [json.loads(ln[len("refit: "):]) for ln in r.stdout.splitlines() if ln.startswith("refit: ")]
    assert len(refit) == 1 and r.stdout.index("merge: ") < r.stdout.index("refit: ")           # the refit corrects the parents
    assert js[0]["met"] is True and rows(out) == js[0]["after"] <= 2600 < js[0]["before"]


def test_cli_merge_batch(glb, tmp_path):
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(out_dir), "--density", str(R), "--format", "1", "--merge-level", "7"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = [json.loads(ln[len("merge: "):]) for ln in r.stdout.splitlines() if ln.startswith("merge: ")]
    assert len(js) == 1 and js[0]["level"] == 7 and rows(str(out_dir / "two.ply")) == js[0]["after"] < js[0]["before"]
    report = [ln for ln in r.stdout.splitlines() if "two.glb ->" in ln]
    assert len(report) == 1 and " ms, merge " in report[0]


def test_cli_merge_usage_errors(glb, tmp_path):
    out = str(tmp_path / "e.ply")
    for bad in (["--merge-level", "3", "--gpus", "2"], ["--merge-level", "11"], ["--merge-level", "-1"], ["--merge-to", "0"], ["--merge-level"],
                ["--merge-level", "3", "--merge-to", "100"], ["--merge-level", "3", "--merge-group", "1"], ["--merge-level", "3", "--merge-group", "65"],
                ["--merge-level", "3", "--merge-dot", "nan"]):
        r, _ = run(glb, out, *bad)
        assert r.returncode == 2 and "usage:" in r.stderr, (bad, r.returncode, r.stderr[:200])
