"""-m gpu: `mesh2splat in.glb out.ply --lod-levels a,b,... --lod-pixels t [--view-distance f] --preview ... | --score K`: the integers
of the `lod:` line against Converter.lod_build / .lod_select for the same cameras, --view-distance, --batch, and the usage errors."""
import json
import os
import subprocess

import numpy as np
import pytest

from mesh2splat_amd import _lib, gltf_io, lod, synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.score import camera_from_eye, orbit_eye, preview_rule

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
R, W, H = 32, 96, 64
LEVELS = (3, 5, 7, 10)
FIELDS = {"levels", "nodes", "per_level_nodes", "skipped", "tau_px", "build_ms", "views"}


def scene():
    return synth.sphere_row(2, n=4, tex_size=16)


@pytest.fixture(scope="module")
def glb(tmp_path_factory, hiplib):
    path = str(tmp_path_factory.mktemp("lod") / "two.glb")
    gltf_io.write_glb(scene(), path)
    return path


def cameras(K, factor=1.0, preview=True):
    """the command line's cameras: the preview's, then the K of --score, at `factor` x the rule's distance with the far plane as much further"""
    ctr, dist, near, far = preview_rule(scene())
    out = [camera_from_eye(orbit_eye(ctr, dist * factor, 0, 1), ctr, near, far * factor, W, H)] if preview else []
    return out + [camera_from_eye(orbit_eye(ctr, dist * factor, k, K), ctr, near, far * factor, W, H) for k in range(K)]


@pytest.fixture(scope="module")
def tree(hiplib):
    """the same tree through the Python interface, and a tau_px that splits the leaves for the preview camera: the median over the
    leaves of e * focal / distance (conversion records store their edges in units the viewer divides by the resolutionTarget, so the
    pin's pixels are not the screen's)"""
    c = Converter(0)
    c.upload_scene(scene())
    c.convert(R)
    build = c.lod_build(LEVELS, 4, 0.5)
    b = c.download_lod(2)[:build["leaves"]].astype(np.float64)
    cam = cameras(0)[0]
    d = np.sqrt(((b[:, 0:3] - np.array(lod.camera_position(cam.view_mat))) ** 2).sum(1))
    tau = float(np.float32(np.median(b[:, 3] * lod.focal_px(cam.proj_mat, H) / d)))
    yield c, build, tau
    c.close()


def expected(c, cams, tau, dry=False):
    out = []
    for cam in cams:
        got = c.lod_select(lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H), tau, cam.near, dry_run=dry)
        out.append({"selected": got["selected"], "per_level": got["per_level"]})
    return out


def run(glb, out, *args):
    r = subprocess.run([EXE, glb, out, "--density", str(R), "--format", "1", "--preview-size", f"{W}x{H}", *args], capture_output=True, text=True, timeout=300)
    return r, [json.loads(ln[len("lod: "):]) for ln in r.stdout.splitlines() if ln.startswith("lod: ")]


def lod_args(tau):
    return ["--lod-levels", ",".join(str(v) for v in LEVELS), "--lod-pixels", f"{tau:.9g}"]


def test_cli_lod_line_against_the_python_interface(glb, tree, tmp_path):
    c, build, tau = tree
    out, png = str(tmp_path / "l.ply"), str(tmp_path / "l.png")
    for factor in (1.0, 4.0):
        extra = [] if factor == 1.0 else ["--view-distance", str(factor)]
        r, js = run(glb, out, *lod_args(tau), "--preview", png, "--score", "3", *extra)
        assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
        j = js[0]
        assert set(j) == FIELDS and j["levels"] == list(LEVELS) and np.float32(j["tau_px"]) == np.float32(tau) and j["build_ms"] > 0
        assert j["nodes"] == build["nodes"] and j["per_level_nodes"] == list(np.diff(build["first"])) and j["skipped"] == build["skipped"]
        assert j["views"] == expected(c, cameras(3, factor), tau)
        assert gltf_io.read_ply(out)[0].shape[0] == build["leaves"]                  # the file keeps the full records
        assert os.path.getsize(png) > 0
        if factor == 1.0:
            near = j["views"][0]
            assert 0 < near["selected"] < build["leaves"] and sum(1 for v in near["per_level"] if v) >= 2
        else:
            assert j["views"][0]["selected"] < near["selected"]                      # four times as far: a coarser cut


def test_cli_view_distance_one_changes_no_byte(glb, tmp_path):
    outs = []
    for k, extra in enumerate(([], ["--view-distance", "1"], ["--view-distance", "2"])):
        out, png = str(tmp_path / f"v{k}.ply"), str(tmp_path / f"v{k}.png")
        r, js = run(glb, out, "--preview", png, "--preview-mode", "6", *extra)
        assert r.returncode == 0 and not js, r.stdout + r.stderr
        outs.append((open(png, "rb").read(), open(out, "rb").read(), [ln for ln in r.stdout.splitlines() if ln.startswith(("preview camera:", "preview light:"))]))
    assert outs[0] == outs[1]
    assert outs[2][1] == outs[0][1] and outs[2][0] != outs[0][0] and outs[2][2][0] != outs[0][2][0]


def test_cli_lod_batch(glb, tree, tmp_path):
    c, build, tau = tree
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(out_dir), "--density", str(R), "--format", "1", "--preview-size", f"{W}x{H}",
                        *lod_args(tau), "--score", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = [json.loads(ln[len("lod: "):]) for ln in r.stdout.splitlines() if ln.startswith("lod: ")]
    assert len(js) == 1 and js[0]["nodes"] == build["nodes"] and js[0]["views"] == expected(c, cameras(2, preview=False), tau, dry=True)
    assert gltf_io.read_ply(str(out_dir / "two.ply"))[0].shape[0] == build["leaves"]


def test_cli_lod_usage_errors(glb, tmp_path):
    out, png = str(tmp_path / "e.ply"), str(tmp_path / "e.png")
    ok = ["--lod-levels", "1,2", "--lod-pixels", "1"]
    for bad in (ok, ["--lod-levels", "1,2", "--preview", png], ["--lod-pixels", "1", "--preview", png], [*ok, "--score", "2", "--gpus", "2"],
                ["--lod-levels", "2,1", "--lod-pixels", "1", "--score", "2"], ["--lod-levels", "11", "--lod-pixels", "1", "--score", "2"],
                ["--lod-levels", "1,,2", "--lod-pixels", "1", "--score", "2"], ["--lod-levels", ",".join(["1"] * 17), "--lod-pixels", "1", "--score", "2"],
                ["--lod-levels", "1", "--lod-pixels", "-1", "--score", "2"], ["--lod-levels", "1", "--lod-pixels", "nan", "--score", "2"],
                ["--preview", png, "--view-distance", "0.2"], ["--preview", png, "--view-distance", "65"], ["--preview", png, "--view-distance", "nan"]):
        r, _ = run(glb, out, *bad)
        assert r.returncode == 2 and "usage:" in r.stderr, (bad, r.returncode, r.stderr[:200])
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(tmp_path), *ok, "--preview", png], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage:" in r.stderr                                # a batch draws no preview: no camera
