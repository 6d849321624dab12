"""-m gpu: `mesh2splat in.glb out.ply --lod-levels a,b,... --lod-pixels t | --lod-budget N --lod-blend b --preview ... | --score K`: the
`lod:` line against Converter.lod_select / .lod_select_budget with blend= for the same cameras, the field sets with and without the flag,
--batch, and the usage errors."""
import json
import os
import subprocess

import numpy as np
import pytest

from mesh2splat_amd import gltf_io, lod
from mesh2splat_amd.converter import Converter
from test_gpu_lod_budget_cli import EXE, FIELDS, H, LEVELS, LV, R, W, cameras, run, scene, views_of

pytestmark = pytest.mark.gpu
BAND = 0.5


@pytest.fixture(scope="module")
def glb(tmp_path_factory, hiplib):
    path = str(tmp_path_factory.mktemp("lodblend") / "two.glb")
    gltf_io.write_glb(scene(), path)
    return path


@pytest.fixture(scope="module")
def tree(hiplib):
    """the same tree through the Python interface, a budget between the last level and the leaves and the tau it gets for the preview camera"""
    c = Converter(0)
    c.upload_scene(scene())
    c.convert(R)
    build = c.lod_build(LEVELS, 4, 0.5)
    budget = (build["leaves"] + build["nodes"] - build["first"][-2]) // 2
    cam = cameras(0)[0]
    free = c.lod_select_budget(lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H), budget, near=cam.near, dry_run=True)
    assert free["tau_px"] > 0 and free["met"]
    yield c, build, budget, float(np.float32(free["tau_px"]))
    c.close()


def test_cli_lod_blend_with_lod_pixels_against_the_python_interface(glb, tree, tmp_path):
    c, build, budget, tau = tree
    out, png = str(tmp_path / "l.ply"), str(tmp_path / "l.png")
    r, js = run(glb, out, *LV, "--lod-pixels", f"{tau:.9g}", "--lod-blend", str(BAND), "--preview", png, "--score", "2")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    j = js[0]
    assert set(j) == FIELDS | {"blend"} and j["blend"] == BAND and j["nodes"] == build["nodes"]
    blended = 0
    for v, cam in zip(j["views"], cameras(2)):
        got = c.lod_select(lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H), tau, cam.near, blend=BAND)
        assert set(v) == {"selected", "per_level", "blended", "blend_ms"}
        assert (v["selected"], v["per_level"], v["blended"]) == (got["selected"], got["per_level"], got["blend"]["blended"])
        assert got["blend"]["records"] == got["selected"] and v["blend_ms"] >= 0
        blended += v["blended"]
    assert blended > 0 and gltf_io.read_ply(out)[0].shape[0] == build["leaves"] and os.path.getsize(png) > 0


def test_cli_lod_blend_with_lod_budget_against_the_python_interface(glb, tree, tmp_path):
    c, build, budget, tau = tree
    out = str(tmp_path / "b.ply")
    r, js = run(glb, out, *LV, "--lod-budget", str(budget), "--lod-blend", str(BAND), "--score", "3")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    j = js[0]
    assert set(j) == FIELDS | {"budget", "blend"} and j["blend"] == BAND and j["budget"] == budget
    for v, cam in zip(views_of(j), cameras(3, preview=False)):
        got = c.lod_select_budget(lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H), budget, near=cam.near, blend=BAND)
        assert set(v) == {"selected", "per_level", "tau_px", "met", "selected_finer", "blended", "blend_ms"}
        assert (v["selected"], v["per_level"], v["tau_px"], v["blended"]) == (got["selected"], got["per_level"], got["tau_px"], got["blend"]["blended"])


def test_cli_line_without_the_flag_is_what_it_was(glb, tree, tmp_path):
    c, build, budget, tau = tree
    r, js = run(glb, str(tmp_path / "p.ply"), *LV, "--lod-pixels", f"{tau:.9g}", "--score", "2")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    assert set(js[0]) == FIELDS and all(set(v) == {"selected", "per_level"} for v in js[0]["views"])


def test_cli_lod_blend_batch_reports_the_band_only(glb, tree, tmp_path):
    c, build, budget, tau = tree
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(out_dir), "--density", str(R), "--format", "1", "--preview-size", f"{W}x{H}",
                        *LV, "--lod-pixels", f"{tau:.9g}", "--lod-blend", str(BAND), "--score", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = [json.loads(ln[len("lod: "):]) for ln in r.stdout.splitlines() if ln.startswith("lod: ")]
    assert len(js) == 1 and set(js[0]) == FIELDS | {"blend"} and js[0]["blend"] == BAND
    assert all(set(v) == {"selected", "per_level"} for v in js[0]["views"])         # dry runs: nothing is blended


def test_cli_lod_blend_usage_errors(glb, tmp_path):
    out = str(tmp_path / "e.ply")
    ok = [*LV, "--lod-pixels", "1", "--score", "2"]
    for bad in (["--lod-blend", "0.5", "--score", "2"], [*ok, "--lod-blend", "0"], [*ok, "--lod-blend", "1.5"], [*ok, "--lod-blend", "-0.5"],
                [*ok, "--lod-blend", "nan"], [*ok, "--lod-blend", "x"], [*ok, "--lod-blend"], [*ok, "--lod-blend", "0.5", "--gpus", "2"]):
        r, _ = run(glb, out, *bad)
        assert r.returncode == 2 and "usage:" in r.stderr, (bad, r.returncode, r.stderr[:200])
    r, js = run(glb, out, *ok, "--lod-blend", "1")
    assert r.returncode == 0 and js[0]["blend"] == 1, r.stdout + r.stderr
