"""-m gpu: `mesh2splat in.glb out.ply --lod-levels a,b,... --lod-pixels t | --lod-budget N --lod-frustum [--lod-guard g]
[--view-distance f] --preview ... | --score K`: the `lod:` line against Converter.lod_select / .lod_select_budget with the same
cameras' frusta, and against the restatement (tests/lod_frustum_ref.py) over the downloaded tree; the field sets with and without the
flag; the usage errors."""
import json
import os
import subprocess

import numpy as np
import pytest

import lod_frustum_ref as fr
from mesh2splat_amd import _lib, gltf_io, lod, synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.score import camera_from_eye, orbit_eye, preview_rule

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
R, W, H = 32, 96, 64
LEVELS = (3, 5, 7, 10)
LV = ["--lod-levels", ",".join(str(v) for v in LEVELS)]
FIELDS = {"levels", "nodes", "per_level_nodes", "skipped", "tau_px", "build_ms", "views"}
EYE = np.eye(4, dtype=np.float32)


def scene():
    return synth.sphere_row(2, n=4, tex_size=16)


@pytest.fixture(scope="module")
def glb(tmp_path_factory, hiplib):
    path = str(tmp_path_factory.mktemp("lodfrustum") / "two.glb")
    gltf_io.write_glb(scene(), path)
    return path


def cameras(K, factor=1.0, preview=True):
    """the command line's cameras: the preview's, then the K of --score, at `factor` x the rule's distance with the far plane as much further"""
    ctr, dist, near, far = preview_rule(scene())
    out = [camera_from_eye(orbit_eye(ctr, dist * factor, 0, 1), ctr, near, far * factor, W, H)] if preview else []
    return out + [camera_from_eye(orbit_eye(ctr, dist * factor, k, K), ctr, near, far * factor, W, H) for k in range(K)]


@pytest.fixture(scope="module")
def tree(hiplib):
    """the same tree through the Python interface, its planes, the tau_px that splits the leaves for the preview camera (as
    tests/test_gpu_lod_cli.py takes it) and a budget between the last level and the leaves"""
    c = Converter(0)
    c.upload_scene(scene())
    c.convert(R)
    build = c.lod_build(LEVELS, 4, 0.5)
    parent, b = c.download_lod(1), c.download_lod(2)
    cam = cameras(0)[0]
    leaves = b[:build["leaves"]].astype(np.float64)
    d = np.sqrt(((leaves[:, 0:3] - np.array(lod.camera_position(cam.view_mat))) ** 2).sum(1))
    tau = float(np.float32(np.median(leaves[:, 3] * lod.focal_px(cam.proj_mat, H) / d)))
    budget = (build["leaves"] + build["nodes"] - build["first"][-2]) // 2
    yield c, build, parent, b, tau, budget
    c.close()


def frustum_of(cam, guard=1.05):
    return lod.frustum_to_c(EYE, cam.view_mat, cam.proj_mat, guard)


def expected(c, cams, tau=None, budget=None, guard=1.05, dry=False):
    out = []
    for cam in cams:
        eye, focal = lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H)
        if budget is None:
            got = c.lod_select(eye, focal, tau, cam.near, dry_run=dry, frustum=frustum_of(cam, guard))
            out.append({k: got[k] for k in ("selected", "per_level", "visible_leaves", "culled")})
        else:
            got = c.lod_select_budget(eye, focal, budget, tau or 0.0, cam.near, dry_run=dry, frustum=frustum_of(cam, guard))
            out.append({k: got[k] for k in ("selected", "per_level", "tau_px", "met", "selected_finer", "visible_leaves", "culled")})
    return out


def run(glb, out, *args):
    r = subprocess.run([EXE, glb, out, "--density", str(R), "--format", "1", "--preview-size", f"{W}x{H}", *args], capture_output=True, text=True, timeout=300)
    return r, [json.loads(ln[len("lod: "):]) for ln in r.stdout.splitlines() if ln.startswith("lod: ")]


def views_of(j):
    """the views with tau_px, where they have one, as the float32 the line's nine digits stand for"""
    return [dict(v, tau_px=float(np.float32(v["tau_px"]))) if "tau_px" in v else v for v in j["views"]]


def test_cli_lod_frustum_with_pixels_against_the_python_interface_and_the_restatement(glb, tree, tmp_path):
    c, build, parent, b, tau, budget = tree
    out, png = str(tmp_path / "l.ply"), str(tmp_path / "l.png")
    for factor in (0.25, 1.0):
        extra = [] if factor == 1.0 else ["--view-distance", str(factor)]
        r, js = run(glb, out, *LV, "--lod-pixels", f"{tau:.9g}", "--lod-frustum", "--preview", png, "--score", "3", *extra)
        assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
        j = js[0]
        assert set(j) == FIELDS | {"frustum"} and np.float32(j["frustum"]) == np.float32(1.05) and np.float32(j["tau_px"]) == np.float32(tau)
        assert j["nodes"] == build["nodes"] and j["per_level_nodes"] == list(np.diff(build["first"]))
        assert all(set(v) == {"selected", "per_level", "visible_leaves", "culled"} for v in j["views"])
        cams = cameras(3, factor)
        assert j["views"] == expected(c, cams, tau)
        want = [fr.select(b, parent, build["first"], lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H), tau, cam.near,
                          (EYE, cam.view_mat, cam.proj_mat, 1.05)) for cam in cams]
        assert [(v["selected"], v["per_level"], v["visible_leaves"], v["culled"]) for v in j["views"]] == \
               [(w["counts"]["selected"], w["per_level"], w["visible_leaves"], w["culled"]) for w in want]
        print(f"--lod-frustum at --view-distance {factor}: {j['views']}")
        if factor == 0.25:
            assert any(w["culled"] > 0 for w in want) and any(v["culled"] > 0 for v in j["views"])   # close in, parts of the row are off screen
        assert gltf_io.read_ply(out)[0].shape[0] == build["leaves"] and os.path.getsize(png) > 0


def test_cli_lod_frustum_with_a_budget_and_a_guard(glb, tree, tmp_path):
    c, build, parent, b, tau, budget = tree
    out, png = str(tmp_path / "b.ply"), str(tmp_path / "b.png")
    for factor, guard in ((0.25, None), (1.0, None), (0.25, 4.0)):
        extra = ([] if factor == 1.0 else ["--view-distance", str(factor)]) + ([] if guard is None else ["--lod-guard", str(guard)])
        r, js = run(glb, out, *LV, "--lod-budget", str(budget), "--lod-frustum", "--preview", png, "--score", "2", *extra)
        assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
        j = js[0]
        assert set(j) == FIELDS | {"budget", "frustum"} and j["budget"] == budget and np.float32(j["frustum"]) == np.float32(guard or 1.05)
        assert all(set(v) == {"selected", "per_level", "tau_px", "met", "selected_finer", "visible_leaves", "culled"} for v in j["views"])
        assert views_of(j) == expected(c, cameras(2, factor), budget=budget, guard=guard or 1.05)
        assert all(v["selected"] <= budget for v in j["views"])
    # --lod-pixels stays the floor
    r, js = run(glb, out, *LV, "--lod-budget", str(budget), "--lod-pixels", "1000", "--lod-frustum", "--score", "1", "--view-distance", "0.25")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    assert views_of(js[0]) == expected(c, cameras(1, 0.25, preview=False), tau=1000.0, budget=budget)
    assert js[0]["views"][0]["tau_px"] == 1000 and js[0]["views"][0]["selected_finer"] == js[0]["views"][0]["selected"]


def test_cli_line_without_the_flag_has_the_fields_it_had(glb, tree, tmp_path):
    c, build, parent, b, tau, budget = tree
    out = str(tmp_path / "p.ply")
    r, js = run(glb, out, *LV, "--lod-pixels", f"{tau:.9g}", "--score", "2", "--view-distance", "0.25")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    assert set(js[0]) == FIELDS and all(set(v) == {"selected", "per_level"} for v in js[0]["views"])
    r, js = run(glb, out, *LV, "--lod-budget", str(budget), "--score", "2")
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    assert set(js[0]) == FIELDS | {"budget"} and all(set(v) == {"selected", "per_level", "tau_px", "met", "selected_finer"} for v in js[0]["views"])


def test_cli_lod_frustum_batch(glb, tree, tmp_path):
    c, build, parent, b, tau, budget = tree
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(out_dir), "--density", str(R), "--format", "1", "--preview-size", f"{W}x{H}",
                        *LV, "--lod-budget", str(budget), "--lod-frustum", "--score", "2", "--view-distance", "0.25"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = [json.loads(ln[len("lod: "):]) for ln in r.stdout.splitlines() if ln.startswith("lod: ")]
    assert len(js) == 1 and js[0]["budget"] == budget and np.float32(js[0]["frustum"]) == np.float32(1.05)
    assert views_of(js[0]) == expected(c, cameras(2, 0.25, preview=False), budget=budget, dry=True)


def test_cli_lod_frustum_usage_errors(glb, tmp_path):
    out, png = str(tmp_path / "e.ply"), str(tmp_path / "e.png")
    ok = [*LV, "--lod-pixels", "1", "--score", "2"]
    for bad in (["--lod-frustum"], ["--lod-frustum", "--preview", png], ["--lod-frustum", "--score", "2"], [*ok, "--lod-guard", "2"],
                [*ok, "--lod-frustum", "--lod-guard", "0.5"], [*ok, "--lod-frustum", "--lod-guard", "nan"], [*ok, "--lod-frustum", "--lod-guard", "inf"],
                [*ok, "--lod-frustum", "--lod-guard", "-1"], [*ok, "--lod-frustum", "--lod-guard"], ["--merge-level", "3", "--lod-frustum"]):
        r, _ = run(glb, out, *bad)
        assert r.returncode == 2 and "usage:" in r.stderr, (bad, r.returncode, r.stderr[:200])
