"""-m gpu: `mesh2splat ... --merge-unsigned-axis` with --merge-level / --merge-to / --lod-levels: the `merge:` and `lod:` JSON lines with
and without the flag (the key appears only with it), against Converter's unsigned_axis for the same inputs, --batch, and the usage errors."""
import json
import os
import subprocess

import numpy as np
import pytest

from mesh2splat_amd import _lib, gltf_io, synth
from mesh2splat_amd.converter import Converter

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
R, W, H = 32, 96, 64
LEVELS = (3, 5, 7, 10)
MERGE_FIELDS = {"level", "max_group", "min_axis_dot", "target", "met", "before", "after", "merged", "invalid", "stage_ms"}
LOD_FIELDS = {"levels", "nodes", "per_level_nodes", "skipped", "tau_px", "build_ms", "views"}


def scene():
    return synth.sphere_row(2, n=4, tex_size=16)


@pytest.fixture(scope="module")
def glb(tmp_path_factory, hiplib):
    path = str(tmp_path_factory.mktemp("merge_unsigned") / "two.glb")
    gltf_io.write_glb(scene(), path)
    return path


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    c.upload_scene(scene())
    yield c
    c.close()


def lines(stdout, tag):
    return [json.loads(ln[len(tag) + 2:]) for ln in stdout.splitlines() if ln.startswith(tag + ": ")]


def run(glb, out, *args):
    return subprocess.run([EXE, glb, out, "--density", str(R), "--format", "1", "--preview-size", f"{W}x{H}", *args], capture_output=True, text=True, timeout=300)


def test_cli_merge_lines_with_and_without_the_flag(glb, conv, tmp_path):
    out = str(tmp_path / "m.ply")
    got = {}
    for flag in (False, True):
        r = run(glb, out, "--merge-level", "7", *(["--merge-unsigned-axis"] if flag else []))
        js = lines(r.stdout, "merge")
        assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
        j = js[0]
        assert set(j) == (MERGE_FIELDS | {"unsigned_axis"} if flag else MERGE_FIELDS) and (not flag or j["unsigned_axis"] is True)
        conv.convert(R)
        want = conv.merge(7, 4, 0.5, unsigned_axis=flag)
        assert {k: j[k] for k in want} == want and gltf_io.read_ply(out)[0].shape[0] == j["after"]
        got[flag] = j
    print("cli --merge-level 7: after", got[False]["after"], "signed,", got[True]["after"], "unsigned")
    assert got[True]["after"] < got[False]["after"]
    # --merge-to: the bisection's dry runs carry the flag too
    N = got[True]["after"]
    r = run(glb, out, "--merge-to", str(N), "--merge-unsigned-axis")
    j = lines(r.stdout, "merge")[0]
    conv.convert(R)
    want = conv.merge_to_budget(N, unsigned_axis=True)
    assert r.returncode == 0 and j["unsigned_axis"] is True and j["target"] == N and (j["level"], j["met"], j["after"]) == (want["level"], want["met"], want["after"])
    assert j["met"] is True and j["level"] <= 7 and j["after"] <= N


def test_cli_lod_line_with_and_without_the_flag(glb, conv, tmp_path):
    out = str(tmp_path / "l.ply")
    args = ["--lod-levels", ",".join(str(v) for v in LEVELS), "--lod-pixels", "40", "--score", "2"]
    nodes = {}
    for flag in (False, True):
        r = run(glb, out, *args, *(["--merge-unsigned-axis"] if flag else []))
        js = lines(r.stdout, "lod")
        assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
        j = js[0]
        assert set(j) == (LOD_FIELDS | {"unsigned_axis"} if flag else LOD_FIELDS) and (not flag or j["unsigned_axis"] is True)
        conv.convert(R)
        build = conv.lod_build(LEVELS, 4, 0.5, unsigned_axis=flag)
        assert j["nodes"] == build["nodes"] and j["per_level_nodes"] == list(np.diff(build["first"])) and j["skipped"] == build["skipped"]
        assert len(j["views"]) == 2 and gltf_io.read_ply(out)[0].shape[0] == build["leaves"]
        nodes[flag] = j["per_level_nodes"]
    print("cli --lod-levels 3,5,7,10: per level", nodes[False], "signed,", nodes[True], "unsigned")
    assert nodes[True][0] == nodes[False][0] and nodes[True][-1] < nodes[False][-1]
    conv.lod_release()


def test_cli_batch_with_the_flag(glb, conv, tmp_path):
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(out_dir), "--density", str(R), "--format", "1", "--preview-size", f"{W}x{H}",
                        "--merge-level", "7", "--merge-unsigned-axis"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = lines(r.stdout, "merge")
    conv.convert(R)
    want = conv.merge(7, 4, 0.5, unsigned_axis=True)
    assert len(js) == 1 and js[0]["unsigned_axis"] is True and js[0]["after"] == want["after"] == gltf_io.read_ply(str(out_dir / "two.ply"))[0].shape[0]
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(out_dir), "--density", str(R), "--format", "1", "--preview-size", f"{W}x{H}",
                        "--lod-levels", "3,5,7,10", "--lod-pixels", "40", "--score", "2", "--merge-unsigned-axis"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = lines(r.stdout, "lod")
    conv.convert(R)
    build = conv.lod_build(LEVELS, 4, 0.5, unsigned_axis=True)
    assert len(js) == 1 and js[0]["unsigned_axis"] is True and js[0]["nodes"] == build["nodes"]
    conv.lod_release()


def test_cli_usage_errors(glb, tmp_path):
    out, png = str(tmp_path / "e.ply"), str(tmp_path / "e.png")
    for bad in (["--merge-unsigned-axis"], ["--merge-unsigned-axis", "--preview", png], ["--merge-unsigned-axis", "--world-units"],
                ["--merge-level", "3", "--merge-unsigned-axis", "--gpus", "2"],
                ["--lod-levels", "1,2", "--lod-pixels", "1", "--score", "2", "--merge-unsigned-axis", "--gpus", "2"]):
        r = run(glb, out, *bad)
        assert r.returncode == 2 and "usage:" in r.stderr, (bad, r.returncode, r.stderr[:200])
