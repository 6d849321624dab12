"""-m gpu: `mesh2splat in.glb out.ply --lod-levels a,b,... --lod-budget N [--lod-pixels t] --preview ... | --score K`: the `lod:` line
against Converter.lod_build / .lod_select_budget for the same cameras, --lod-pixels as the floor, the line without the flag, --batch,
and the usage errors."""
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
    path = str(tmp_path_factory.mktemp("lodbudget") / "two.glb")
    gltf_io.write_glb(scene(), path)
    return path


def cameras(K, preview=True):
    """the command line's cameras: the preview's, then the K of --score"""
    ctr, dist, near, far = preview_rule(scene())
    out = [camera_from_eye(orbit_eye(ctr, dist, 0, 1), ctr, near, far, W, H)] if preview else []
    return out + [camera_from_eye(orbit_eye(ctr, dist, k, K), ctr, near, far, W, H) for k in range(K)]


@pytest.fixture(scope="module")
def tree(hiplib):
    """the same tree through the Python interface, a budget between the last level and the leaves, and a floor above the tau that budget
    gets for the preview camera"""
    c = Converter(0)
    c.upload_scene(scene())
    c.convert(R)
    build = c.lod_build(LEVELS, 4, 0.5)
    budget = (build["leaves"] + build["nodes"] - build["first"][-2]) // 2
    cam = cameras(0)[0]
    free = c.lod_select_budget(lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H), budget, near=cam.near, dry_run=True)
    assert free["tau_px"] > 0 and free["met"] and free["selected"] <= budget < free["selected_finer"]
    yield c, build, budget, float(np.float32(free["tau_px"] * 1.5))
    c.close()


def expected(c, cams, budget, floor=0.0, dry=False):
    out = []
    for cam in cams:
        got = c.lod_select_budget(lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H), budget, floor, cam.near, dry_run=dry)
        out.append({"selected": got["selected"], "per_level": got["per_level"], "tau_px": got["tau_px"], "met": got["met"],
                    "selected_finer": got["selected_finer"]})
    return out


def run(glb, out, *args):
    r = subprocess.run([EXE, glb, out, "--density", str(R), "--format", "1", "--preview-size", f"{W}x{H}", *args], capture_output=True, text=True, timeout=300)
    return r, [json.loads(ln[len("lod: "):]) for ln in r.stdout.splitlines() if ln.startswith("lod: ")]


def views_of(j):
    """the views with tau_px as the float32 the line's nine digits stand for"""
    return [dict(v, tau_px=float(np.float32(v["tau_px"]))) for v in j["views"]]


LV = ["--lod-levels", ",".join(str(v) for v in LEVELS)]


def test_cli_lod_budget_line_against_the_python_interface(glb, tree, tmp_path):
    c, build, budget, floor = tree
    out, png = str(tmp_path / "l.ply"), str(tmp_path / "l.png")
    r, js = run(glb, out, *LV, "--lod-budget", str(budget), "--preview", png, "--score", "3")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    j = js[0]
    assert set(j) == FIELDS | {"budget"} and j["budget"] == budget and j["tau_px"] == 0 and j["levels"] == list(LEVELS)
    assert j["nodes"] == build["nodes"] and j["per_level_nodes"] == list(np.diff(build["first"])) and j["skipped"] == build["skipped"]
    want = expected(c, cameras(3), budget)
    assert views_of(j) == want
    assert all(v["met"] and v["selected"] <= budget < v["selected_finer"] for v in want)
    assert gltf_io.read_ply(out)[0].shape[0] == build["leaves"] and os.path.getsize(png) > 0
    # a budget below the last level: not met, the coarsest cut
    r, js = run(glb, out, *LV, "--lod-budget", "1", "--score", "2")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    assert views_of(js[0]) == expected(c, cameras(2, preview=False), 1)
    # (as many records as the last level has nodes, not always its own: a node with one child is replaced by it at no cost)
    assert all(not v["met"] and v["selected"] == build["nodes"] - build["first"][-2] for v in js[0]["views"])


def test_cli_lod_pixels_is_the_floor(glb, tree, tmp_path):
    c, build, budget, floor = tree
    out, png = str(tmp_path / "f.ply"), str(tmp_path / "f.png")
    r, js = run(glb, out, *LV, "--lod-budget", str(budget), "--lod-pixels", f"{floor:.9g}", "--preview", png)
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    j = js[0]
    assert j["budget"] == budget and np.float32(j["tau_px"]) == np.float32(floor)
    assert views_of(j) == expected(c, cameras(0), budget, floor)
    v = j["views"][0]
    assert np.float32(v["tau_px"]) == np.float32(floor) and v["selected_finer"] == v["selected"] <= budget      # the floor decided


def test_cli_line_without_the_flag_is_what_it_was(glb, tree, tmp_path):
    c, build, budget, floor = tree
    out = str(tmp_path / "p.ply")
    r, js = run(glb, out, *LV, "--lod-pixels", f"{floor:.9g}", "--score", "2")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("lod: ")][0]
    j = js[0]
    assert set(j) == FIELDS and all(set(v) == {"selected", "per_level"} for v in j["views"])
    views = []
    for cam in cameras(2, preview=False):
        got = c.lod_select(lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H), floor, cam.near)
        views.append({"selected": got["selected"], "per_level": got["per_level"]})
    assert j["views"] == views
    # byte for byte the line the parent commit prints: its format string, filled in
    want = ('lod: {"levels": [%s], "nodes": %d, "per_level_nodes": [%s], "skipped": %d, "tau_px": %s, "build_ms": %.4f, "views": [%s]}' %
            (", ".join(str(v) for v in LEVELS), build["nodes"], ", ".join(str(v) for v in np.diff(build["first"])), build["skipped"],
             "%.9g" % float(np.float32(floor)), j["build_ms"],
             ", ".join('{"selected": %d, "per_level": [%s]}' % (v["selected"], ", ".join(str(k) for k in v["per_level"])) for v in views)))
    assert line == want


def test_cli_lod_budget_batch(glb, tree, tmp_path):
    c, build, budget, floor = tree
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(out_dir), "--density", str(R), "--format", "1", "--preview-size", f"{W}x{H}",
                        *LV, "--lod-budget", str(budget), "--score", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = [json.loads(ln[len("lod: "):]) for ln in r.stdout.splitlines() if ln.startswith("lod: ")]
    assert len(js) == 1 and js[0]["nodes"] == build["nodes"] and js[0]["budget"] == budget
    assert views_of(js[0]) == expected(c, cameras(2, preview=False), budget, dry=True)
    assert gltf_io.read_ply(str(out_dir / "two.ply"))[0].shape[0] == build["leaves"]


def test_cli_lod_budget_usage_errors(glb, tmp_path):
    out, png = str(tmp_path / "e.ply"), str(tmp_path / "e.png")
    ok = [*LV, "--lod-budget", "100"]
    for bad in (ok, ["--lod-budget", "100", "--preview", png], ["--lod-budget", "100", "--lod-pixels", "1", "--score", "2"], [*ok, "--score", "2", "--gpus", "2"],
                [*LV, "--lod-budget", "0", "--score", "2"], [*LV, "--lod-budget", "-5", "--score", "2"], [*LV, "--lod-budget", "12x", "--score", "2"],
                [*LV, "--lod-budget", "", "--score", "2"], [*LV, "--lod-budget", "4294967296", "--score", "2"], [*LV, "--score", "2", "--lod-budget"],
                [*ok, "--lod-pixels", "-1", "--score", "2"]):
        r, _ = run(glb, out, *bad)
        assert r.returncode == 2 and "usage:" in r.stderr, (bad, r.returncode, r.stderr[:200])
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(tmp_path), *ok, "--preview", png], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage:" in r.stderr                                # a batch draws no preview: no camera
