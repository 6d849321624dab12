"""-m gpu: `mesh2splat in.glb out.ply --compact`: the file against Converter.export_ply_compact on the same .glb, the JSON line, the
usage errors."""
import json
import os
import subprocess

import pytest

from mesh2splat_amd import _lib, gltf_io, synth
from mesh2splat_amd.converter import Converter

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
R = 64


def test_cli_compact(tmp_path, hiplib):
    glb, out, ref = str(tmp_path / "s.glb"), str(tmp_path / "s.ply"), str(tmp_path / "ref.ply")
    gltf_io.write_glb(synth.sphere_grid(2, n=5, tex_size=32), glb)
    r = subprocess.run([EXE, glb, out, "--density", str(R), "--compact"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("compact: ")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0][len("compact: "):])
    conv = Converter(0)
    try:
        conv.upload_scene(gltf_io.load_glb(glb))
        n = conv.convert(R)
        want = conv.export_ply_compact(ref, 0.65)
    finally:
        conv.close()
    data = open(out, "rb").read()
    assert data == open(ref, "rb").read()
    assert j["rows"] == want["rows"] == n and j["chunks"] == want["chunks"] == (n + 255) // 256 and j["skipped"] == 0
    assert j["bytes"] == len(data) == want["bytes"] and len(j["stage_ms"]) == 4 and all(v >= 0 for v in j["stage_ms"])
    assert data.startswith(b"ply\nformat binary_little_endian 1.0\nelement chunk ")
    # --batch alone: the same file
    bdir, odir = tmp_path / "in", tmp_path / "out"
    bdir.mkdir()
    odir.mkdir()
    os.replace(glb, str(bdir / "s.glb"))
    r = subprocess.run([EXE, "--batch", str(bdir), "--out", str(odir), "--density", str(R), "--compact"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(str(odir / "s.ply"), "rb").read() == data and sum(ln.startswith("compact: ") for ln in r.stdout.splitlines()) == 1


def test_cli_compact_usage_errors(tmp_path, hiplib):
    glb, out = str(tmp_path / "s.glb"), str(tmp_path / "s.ply")
    gltf_io.write_glb(synth.sphere_grid(1, n=4, tex_size=16), glb)
    for bad in (["--compact", "--gpus", "2"], ):
        r = subprocess.run([EXE, glb, out, "--density", "32"] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--compact" in r.stderr, (bad, r.returncode, r.stderr[:200])
    r = subprocess.run([EXE, "--batch", str(tmp_path), "--out", str(tmp_path), "--compact", "--gpus", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2
