"""-m gpu: `mesh2splat in.ply out.ply ...`: a .ply in place of a .glb — the file against what the Python interface produces from the
same input, an SH plane carried through, --budget, --compact, the `ply_in:` / `merge:` JSON lines, `--merge-model` on a .glb, and
the usage errors."""
import json
import os
import subprocess

import numpy as np
import pytest

import merge_gauss_ref as mg
import merge_sh_ref as ms
from mesh2splat_amd import _lib, gltf_io, synth
from mesh2splat_amd.converter import Converter, write_ply

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
F = np.float32
N = 2000
MERGE_FIELDS = {"level", "max_group", "min_axis_dot", "target", "met", "before", "after", "merged", "invalid", "stage_ms"}


def lines(r, key):
    return [json.loads(ln[len(key) + 2:]) for ln in r.stdout.splitlines() if ln.startswith(key + ": ")]


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, hiplib):
    """a standard-layout .ply of three-axis Gaussians without a plane of higher degree, and one with a degree-2 plane"""
    d = tmp_path_factory.mktemp("plyin")
    rec = mg.gauss_records(N, 17, invalid=False)
    rec[:, 8:11] = np.maximum(rec[:, 8:11], F(1e-3))                   # (a file stores log scale)
    rec[:, 7] = np.clip(rec[:, 7], 0.05, 0.95)
    plain, with_sh = str(d / "plain.ply"), str(d / "sh2.ply")
    write_ply(plain, rec, 0, 1.0)
    sh = ms.random_plane(N, 2)
    for ch in range(3):
        sh[:, 3 + 15 * ch + 8:3 + 15 * (ch + 1)] = 0                   # degree 2: 8 coefficients per channel
    assert hiplib.m2s_write_ply_sh(os.fsencode(with_sh), rec.ctypes.data, sh.ctypes.data, N, 1.0) == 0
    return plain, with_sh


def test_cli_merges_a_ply_as_the_python_interface_does(inputs, tmp_path):
    plain, _ = inputs
    out, want = str(tmp_path / "o.ply"), str(tmp_path / "w.ply")
    r = run(plain, out, "--merge-level", "3", "--merge-model", "gaussian")
    assert r.returncode == 0, r.stdout + r.stderr
    pin, mj = lines(r, "ply_in"), lines(r, "merge")
    assert pin == [{"rows": N, "has_pbr": False, "sh_degree": 3}]        # (the standard layout always has its 45 f_rest, zeros here)
    assert len(mj) == 1 and set(mj[0]) == MERGE_FIELDS | {"model", "sigma"} and (mj[0]["model"], mj[0]["sigma"]) == ("gaussian", 1.0)
    rec, _, sh, degree = gltf_io.read_ply_sh(plain)
    c = Converter(0)
    try:
        c.set_merge_model("gaussian", 1.0)
        c.carry_sh = True
        c.upload_records(rec)
        c.upload_sh(sh, degree)
        counts = c.merge(3)
        assert (mj[0]["before"], mj[0]["after"], mj[0]["merged"]) == (N, counts["after"], counts["merged"]) and counts["after"] < N
        got, plane = c.download(), c.download_sh()
    finally:
        c.close()
    assert _lib.load().m2s_write_ply_sh(os.fsencode(want), got.ctypes.data, plane.ctypes.data, len(got), 1.0) == 0
    assert open(out, "rb").read() == open(want, "rb").read()
    # the footprint on the same file: another result, and no model keys without the flag
    r = run(plain, out, "--merge-level", "3")
    assert r.returncode == 0 and set(lines(r, "merge")[0]) == MERGE_FIELDS
    assert open(out, "rb").read() != open(want, "rb").read()
    r = run(plain, out, "--merge-to", str(N // 2), "--merge-model", "gaussian", "--merge-sigma", "0.5", "--format", "1")
    assert r.returncode == 0 and lines(r, "merge")[0]["sigma"] == 0.5 and gltf_io.read_ply(out)[0].shape[0] == lines(r, "merge")[0]["after"]


def test_cli_carries_a_degree_two_plane(inputs, tmp_path):
    _, with_sh = inputs
    out = str(tmp_path / "o.ply")
    r = run(with_sh, out, "--merge-level", "10", "--merge-group", "8", "--merge-dot", "-2", "--merge-model", "gaussian")
    assert r.returncode == 0, r.stdout + r.stderr
    after = lines(r, "merge")[0]["after"]
    got, _, plane, degree = gltf_io.read_ply_sh(out)
    assert len(got) == after < N and plane.shape == (after, 48) and degree == 3
    assert np.abs(plane[:, 3:11]).max() > 0 and not plane[:, 11:18].any()        # degree 2 went in, degree 2 came out
    # ... the rows pin 5sg makes of the input's
    rec, _, sh, _ = gltf_io.read_ply_sh(with_sh)
    perm, heads = mg.segment_heads(rec, 10, 8, -2.0)
    wplane, pinfo = mg.merge_plane(rec, sh, perm, heads)
    assert ms.compare(plane, wplane, pinfo) <= ms.PLANE_ULPS_BAR
    # a budget by area in front of the merge keeps the plane too
    r = run(with_sh, out, "--budget", str(N // 2), "--merge-level", "3")
    assert r.returncode == 0 and lines(r, "budget")[0]["kept"] == N // 2 and r.stdout.index("budget: ") < r.stdout.index("merge: ")
    got, _, plane, _ = gltf_io.read_ply_sh(out)
    assert len(got) == lines(r, "merge")[0]["after"] and np.abs(plane[:, 3:11]).max() > 0


def test_cli_compact_on_a_ply_input(inputs, tmp_path):
    plain, with_sh = inputs
    out = str(tmp_path / "c.ply")
    r = run(plain, out, "--compact", "--merge-level", "3", "--merge-model", "gaussian")
    assert r.returncode == 0, r.stdout + r.stderr
    cj = lines(r, "compact")
    assert len(cj) == 1 and cj[0]["rows"] == lines(r, "merge")[0]["after"] and cj[0]["bytes"] == os.path.getsize(out)
    back, _ = gltf_io.read_ply(out)
    assert len(back) == cj[0]["rows"]
    # the scales come back as they went in (multiplier 1), to the compact layout's quantisation
    r = run(plain, out, "--compact")
    assert r.returncode == 0
    back, _ = gltf_io.read_ply(out)
    src, _ = gltf_io.read_ply(plain)
    assert len(back) == N and abs(np.log(back[:, 8:11]).mean() - np.log(src[:, 8:11]).mean()) < 0.05
    r = run(with_sh, out, "--compact")
    assert r.returncode == 0 and lines(r, "compact")[0]["rows"] == N


def test_cli_merge_model_on_a_glb(tmp_path):
    glb = str(tmp_path / "two.glb")
    gltf_io.write_glb(synth.sphere_row(2, n=4, tex_size=16), glb)
    out = str(tmp_path / "g.ply")
    base = [glb, out, "--density", "32", "--format", "1", "--world-units", "--merge-level", "6"]
    r = run(*base, "--merge-model", "gaussian", "--merge-sigma", "0.65")
    assert r.returncode == 0, r.stdout + r.stderr
    j = lines(r, "merge")[0]
    assert j["model"] == "gaussian" and F(j["sigma"]) == F(0.65) and j["after"] < j["before"]       # (nine digits: the float, not its double)
    r0 = run(*base)
    assert r0.returncode == 0 and set(lines(r0, "merge")[0]) == MERGE_FIELDS
    r = run(glb, out, "--density", "32", "--lod-levels", "3,6", "--lod-pixels", "2", "--score", "1", "--merge-model", "gaussian")
    assert r.returncode == 0, r.stdout + r.stderr
    lj = lines(r, "lod")[0]
    assert (lj["model"], lj["sigma"]) == ("gaussian", 1.0)


@pytest.mark.parametrize("extra", (("--preview", "p.png"), ("--score", "2"), ("--refit", "1"), ("--prune", "2"), ("--bake-light",), ("--split-screen", "0.5"),
                                   ("--mesh-depth-test",), ("--lod-levels", "3", "--lod-pixels", "1"), ("--lod-pixels", "1"), ("--lod-budget", "10"),
                                   ("--lod-frustum",), ("--lod-occlusion",), ("--lod-blend", "0.5"), ("--lod-ply", "c.ply"), ("--world-units",),
                                   ("--density", "32"), ("--quality", "0.5"), ("--max-res", "64"), ("--std", "0.5"), ("--cap", "10"), ("--gpus", "2"),
                                   ("--batch", ".", "--out", "."),
                                   ("--merge-model", "gaussian"), ("--merge-sigma", "0.5", "--merge-level", "3"),
                                   ("--merge-model", "round", "--merge-level", "3"), ("--merge-model", "gaussian", "--merge-sigma", "0", "--merge-level", "3")))
def test_cli_usage_errors_with_a_ply_input(inputs, tmp_path, extra):
    plain, _ = inputs
    out = str(tmp_path / "never.ply")
    r = run(plain, out, *extra)
    assert r.returncode == 2 and "usage: mesh2splat" in r.stderr and not os.path.exists(out), (extra, r.stdout, r.stderr)


def test_cli_blend_takes_no_gaussian_tree_and_a_missing_file_is_an_error(tmp_path):
    r = run("x.glb", "y.ply", "--lod-levels", "3", "--lod-pixels", "1", "--score", "1", "--lod-blend", "0.5", "--merge-model", "gaussian")
    assert r.returncode == 2
    r = run(str(tmp_path / "missing.ply"), str(tmp_path / "o.ply"), "--merge-level", "3")
    assert r.returncode == 1 and "missing.ply" in r.stderr
