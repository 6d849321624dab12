"""-m gpu: `mesh2splat in.glb out.ply --world-units ...`: the `world_units:` line against Converter.to_world_units, a level-of-detail cut
over the unit quad that is mixed at a --lod-pixels counted in screen pixels, --batch, the usage error with --gpus, and that the export
at a power-of-two density is the same file with and without it."""
import json
import os
import subprocess

import pytest

from mesh2splat_amd import _lib, gltf_io, synth
from mesh2splat_amd.converter import Converter

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
R, W, H = 64, 96, 64


@pytest.fixture(scope="module")
def glb(tmp_path_factory, hiplib):
    path = str(tmp_path_factory.mktemp("wu") / "quad.glb")
    gltf_io.write_glb(synth.unit_quad(), path)
    return path


def run(glb, out, *args, density=R):
    r = subprocess.run([EXE, glb, out, "--density", str(density), "--format", "1", "--preview-size", f"{W}x{H}", *args], capture_output=True, text=True, timeout=300)
    return r


def lines(r, tag):
    return [json.loads(ln[len(tag) + 2:]) for ln in r.stdout.splitlines() if ln.startswith(tag + ": ")]


def test_cli_world_units_line_against_the_python_interface(glb, tmp_path):
    c = Converter(0)
    try:
        c.upload_scene(gltf_io.load_glb(glb))
        c.convert(R)
        want = c.to_world_units()
    finally:
        c.close()
    r = run(glb, str(tmp_path / "a.ply"), "--world-units")
    assert r.returncode == 0, r.stdout + r.stderr
    js = lines(r, "world_units")
    assert len(js) == 1 and set(js[0]) == {"records", "previous_R", "ms"}
    assert js[0]["records"] == want["records"] == R * R and js[0]["previous_R"] == want["previous_R"] == R and js[0]["ms"] > 0


def test_cli_export_is_the_same_file_with_and_without(glb, tmp_path):
    """density 64: the division and std / 64 are exact scalings"""
    for fmt in ("0", "1", "2"):
        a, b = str(tmp_path / f"a{fmt}.ply"), str(tmp_path / f"b{fmt}.ply")
        ra = subprocess.run([EXE, glb, a, "--density", str(R), "--format", fmt], capture_output=True, text=True, timeout=300)
        rb = subprocess.run([EXE, glb, b, "--density", str(R), "--format", fmt, "--world-units"], capture_output=True, text=True, timeout=300)
        assert ra.returncode == 0 and rb.returncode == 0, ra.stderr + rb.stderr
        assert not lines(ra, "world_units") and len(lines(rb, "world_units")) == 1
        assert open(a, "rb").read() == open(b, "rb").read(), fmt


def test_cli_lod_over_world_units_takes_a_mixed_cut(glb, tmp_path):
    """--lod-pixels 4 on the quad: without --world-units the preview camera draws every leaf (the pin's pixels are 64ths of the screen's),
    with it nodes of several levels; the previews are drawn either way"""
    lod = ["--lod-levels", "4,5,6,7,8,9,10", "--lod-pixels", "4"]
    png = str(tmp_path / "p.png")
    r = run(glb, str(tmp_path / "w.ply"), "--world-units", *lod, "--preview", png, "--score", "2")
    assert r.returncode == 0, r.stdout + r.stderr
    j = lines(r, "lod")
    assert len(j) == 1 and len(lines(r, "world_units")) == 1 and os.path.getsize(png) > 0
    assert r.stdout.index("world_units: ") < r.stdout.index("lod: ")
    assert j[0]["per_level_nodes"][0] == R * R and len(j[0]["per_level_nodes"]) >= 3
    for view in j[0]["views"]:
        assert sum(1 for v in view["per_level"] if v) >= 2 and 0 < view["selected"] < R * R, view
    assert len(lines(r, "score")) == 1
    r0 = run(glb, str(tmp_path / "s.ply"), *lod, "--preview", png)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    v0 = lines(r0, "lod")[0]["views"][0]
    assert v0["selected"] == v0["per_level"][0] == R * R
    assert open(str(tmp_path / "w.ply"), "rb").read() == open(str(tmp_path / "s.ply"), "rb").read()     # the file keeps the full records


def test_cli_world_units_in_front_of_the_other_stages(glb, tmp_path):
    """--merge-level 5 behind it (the first level whose cells hold more than one record of this quad): its 2 x 2 blocks merge as a
    quadtree's (1088 parents, tests/test_worldunits_ref.py); --prune and --refit take the divisor from the context and see what they saw
    without the pass"""
    r = run(glb, str(tmp_path / "m.ply"), "--world-units", "--merge-level", "5", "--compact")
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.index("world_units: ") < r.stdout.index("merge: ") < r.stdout.index("compact: ")
    assert lines(r, "merge")[0]["before"] == R * R and lines(r, "merge")[0]["after"] == 1088
    outs = []
    for extra in ([], ["--world-units"]):
        r = run(glb, str(tmp_path / f"p{len(extra)}.ply"), *extra, "--prune", "3", "--refit", "2", "--score", "2")
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append((lines(r, "prune"), lines(r, "refit"), lines(r, "score"), open(str(tmp_path / f"p{len(extra)}.ply"), "rb").read()))
    assert outs[0] == outs[1]


def test_cli_world_units_batch_and_usage(glb, tmp_path):
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(out_dir), "--density", str(R), "--format", "1", "--world-units"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = lines(r, "world_units")
    assert len(js) == 1 and js[0]["records"] == R * R and js[0]["previous_R"] == R
    single = str(tmp_path / "single.ply")
    assert run(glb, single).returncode == 0
    assert open(str(out_dir / "quad.ply"), "rb").read() == open(single, "rb").read()
    for bad in (["--gpus", "2", "--world-units"], ["--world-units", "1"]):
        r = run(glb, str(tmp_path / "e.ply"), *bad)
        assert r.returncode == 2 and "usage:" in r.stderr, (bad, r.returncode, r.stderr[:200])
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(out_dir), "--gpus", "2", "--world-units"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage:" in r.stderr
    assert "--world-units" in r.stderr and "screen pixels" in r.stderr
