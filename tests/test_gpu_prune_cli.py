"""-m gpu: `mesh2splat in.glb out.ply --prune K`: the JSON record, the rows of the .ply, the cameras against
mesh2splat_amd.prune.orbit_cameras, and the usage errors."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from mesh2splat_amd import _lib, gltf_io, synth
from mesh2splat_amd.prune import orbit_cameras

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
W, H, R = 96, 64, 64


def test_cli_prune(tmp_path, hiplib):
    glb, out = str(tmp_path / "s.glb"), str(tmp_path / "s.ply")
    scene = synth.sphere_grid(2, n=5, tex_size=32)
    gltf_io.write_glb(scene, glb)
    r = subprocess.run([EXE, glb, out, "--density", str(R), "--preview-size", f"{W}x{H}", "--prune", "4", "--prune-elevations", "-20,30"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("prune: ")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0][len("prune: "):])
    assert j["views"] == 4 and j["elevations"] == [-20, 30] and j["size"] == [W, H] and j["density"] == R and len(j["eyes"]) == 8
    assert j["kept"] + j["dropped_weight"] + j["dropped_pixels"] == j["before"] and 0 < j["kept"] <= j["before"]
    assert j["min_pixels"] == 1 and abs(j["min_weight"] - 1 / 255) < 1e-8 and abs(j["count_weight"] - 1 / 255) < 1e-8
    cams = orbit_cameras(gltf_io.load_glb(glb), 4, W, H, (-20.0, 30.0))
    assert np.allclose(np.array(j["eyes"]), np.array([c.eye for c in cams]), rtol=0, atol=1e-5)
    head = open(out, "rb").read(4096).split(b"end_header")[0].decode()
    assert int(re.search(r"element vertex (\d+)", head).group(1)) == j["kept"]
    assert f"({j['kept']} stored)" in r.stdout


def test_cli_prune_usage_errors(tmp_path, hiplib):
    glb, out = str(tmp_path / "s.glb"), str(tmp_path / "s.ply")
    gltf_io.write_glb(synth.sphere_grid(1, n=4, tex_size=16), glb)
    base = [EXE, glb, out, "--density", "32", "--preview-size", "64x48"]
    for bad in (["--prune", "2", "--gpus", "2"], ["--prune", "0"], ["--prune", "2", "--prune-elevations", "90"], ["--prune", "2", "--prune-elevations", "10,,20"],
                ["--prune", "2", "--prune-weight", "-1"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, (bad, r.returncode, r.stderr[:200])
