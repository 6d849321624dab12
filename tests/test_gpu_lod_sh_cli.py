"""-m gpu: `mesh2splat in.glb out.ply --lod-levels ... --preview view.png --lod-ply cut.ply [--bake-light]`: the file the preview camera's
cut is written to against the Python interface (byte for byte: with --bake-light the records and the carried SH plane through
export_ply_sh, without it export_ply in --format), the key sets of the `lod:` line with and without the option, and the usage errors."""
import json
import os
import subprocess

import numpy as np
import pytest

from mesh2splat_amd import gltf_io, lod
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prepass import PrepassParams
from mesh2splat_amd.score import orbit_eye, preview_rule
from test_gpu_lod_cli import EXE, FIELDS, H, LEVELS, R, W, cameras, glb, lod_args, scene, tree  # noqa: F401 (glb, tree: fixtures)

pytestmark = pytest.mark.gpu
LIGHT = (1.5, 2.0, 2.5, 9.0)


def run(glb, out, fmt, *args):
    r = subprocess.run([EXE, glb, out, "--density", str(R), "--format", str(fmt), "--preview-size", f"{W}x{H}", *args], capture_output=True, text=True,
                       timeout=300)
    return r, [json.loads(ln[len("lod: "):]) for ln in r.stdout.splitlines() if ln.startswith("lod: ")]


def ply_header(path):
    head = open(path, "rb").read().split(b"end_header\n", 1)[0].decode().splitlines()
    rows = [int(ln.split()[2]) for ln in head if ln.startswith("element vertex")][0]
    return rows, [ln.split()[2] for ln in head if ln.startswith("property")]


def test_lod_ply_without_a_bake_is_the_cut_in_the_chosen_format(glb, tree, tmp_path):
    _, build, tau = tree
    out, png, cut, py = (str(tmp_path / n) for n in ("o.ply", "o.png", "cut.ply", "py.ply"))
    r, js = run(glb, out, 1, *lod_args(tau), "--preview", png, "--lod-ply", cut)
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    j = js[0]
    assert set(j) == FIELDS | {"cut_ply"} and j["cut_ply"] == cut
    cam = cameras(0)[0]
    c = Converter(0)
    try:
        c.upload_scene(gltf_io.load_glb(glb))                                        # (the file's own floats, as the command line reads them)
        c.convert(R)
        full = str(tmp_path / "full.ply")
        c.export_ply(full, 1, 0.65)
        assert open(full, "rb").read() == open(out, "rb").read()
        assert c.lod_build(LEVELS, 4, 0.5)["nodes"] == j["nodes"] == build["nodes"]
        got = c.lod_select(lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H), tau, cam.near)
        assert j["views"] == [{"selected": got["selected"], "per_level": got["per_level"]}] and 0 < got["selected"] < build["leaves"]
        c.export_ply(py, 1, 0.65)
    finally:
        c.close()
    assert open(cut, "rb").read() == open(py, "rb").read()
    rows, props = ply_header(cut)
    assert rows == got["selected"] and not any(p.startswith("f_rest") for p in props)
    # without the option: the key set and the files of today
    out2, png2 = str(tmp_path / "p.ply"), str(tmp_path / "p.png")
    r2, js2 = run(glb, out2, 1, *lod_args(tau), "--preview", png2)
    assert r2.returncode == 0 and set(js2[0]) == FIELDS and js2[0]["views"] == j["views"]
    assert open(out2, "rb").read() == open(out, "rb").read() and open(png2, "rb").read() == open(png, "rb").read()


def test_lod_ply_with_a_bake_carries_the_plane(glb, tree, tmp_path):
    _, build, tau = tree
    out, png, cut, py = (str(tmp_path / n) for n in ("o.ply", "o.png", "cut.ply", "py.ply"))
    bake = ["--bake-light", "--bake-degree", "2", "--light", ",".join(str(v) for v in LIGHT)]
    r, js = run(glb, out, 0, *bake, *lod_args(tau), "--preview", png, "--lod-ply", cut)
    assert r.returncode == 0 and len(js) == 1, r.stdout + r.stderr
    j = js[0]
    assert set(j) == FIELDS | {"cut_ply", "sh_degree"} and j["cut_ply"] == cut and j["sh_degree"] == 2
    # --bake-light --lod-levels without --lod-ply: byte for byte what it was, and the old key set
    out0, png0 = str(tmp_path / "b.ply"), str(tmp_path / "b.png")
    r0, js0 = run(glb, out0, 0, *bake, *lod_args(tau), "--preview", png0)
    assert r0.returncode == 0 and set(js0[0]) == FIELDS and js0[0]["views"] == j["views"]
    assert open(out0, "rb").read() == open(out, "rb").read() and open(png0, "rb").read() == open(png, "rb").read()
    # the same through the Python interface: the command line's bake (tests/test_gpu_bake.py's recipe), the tree with the switch on, the cut
    cam = cameras(0)[0]
    ctr, dist, near, far = preview_rule(scene())
    eye = orbit_eye(ctr, dist, 0, 1)
    c = Converter(0)
    try:
        c.carry_sh = True
        c.upload_scene(gltf_io.load_glb(glb))                                        # (the file's own floats, as the command line reads them)
        c.convert(R)
        pp = PrepassParams(view_mat=cam.view_mat, proj_mat=cam.proj_mat, renderer_resolution=(W, H), near_plane=near, far_plane=far, resolution_target=R)
        lp = LightParams(LIGHT[:3], (1.0, 1.0, 1.0), LIGHT[3], tuple(float(v) for v in eye), near, far, 6, (W, H), 1024, False)
        c.shadow(pp, lp, download=False)
        c.bake_light(BakeParams(degree=2), lp, download=False)
        full = str(tmp_path / "full.ply")
        c.export_ply_sh(full, 0.65)
        assert open(full, "rb").read() == open(out, "rb").read()                     # (the bake is the command line's: the comparison below means something)
        assert c.lod_build(LEVELS, 4, 0.5)["nodes"] == j["nodes"]
        got = c.lod_select(lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H), tau, cam.near)
        assert j["views"] == [{"selected": got["selected"], "per_level": got["per_level"]}]
        assert c.sh_plane_info() == {"rows": got["selected"], "degree": 2}
        c.export_ply_sh(py, 0.65)
        assert open(cut, "rb").read() == open(py, "rb").read()
        rows, props = ply_header(cut)
        assert rows == got["selected"] and sum(1 for p in props if p.startswith("f_rest_")) == 45 and sum(1 for p in props if p.startswith("f_dc_")) == 3
        sh = c.download_sh()
        assert np.isfinite(sh).all() and sh[:, 3:].any() and not sh[:, [3 + 15 * ch + k for ch in range(3) for k in range(8, 15)]].any()   # degree 2
    finally:
        c.close()


def test_lod_ply_usage_errors(glb, tmp_path):
    out, png, cut = str(tmp_path / "e.ply"), str(tmp_path / "e.png"), str(tmp_path / "e_cut.ply")
    ok = ["--lod-levels", "1,2", "--lod-pixels", "1"]
    for bad in (["--preview", png, "--lod-ply", cut],                                # no --lod-levels
                [*ok, "--score", "2", "--lod-ply", cut],                             # no --preview
                [*ok, "--preview", png, "--lod-ply", cut, "--gpus", "2"],
                [*ok, "--preview", png, "--lod-ply"]):                               # no file name
        r, _ = run(glb, out, 1, *bad)
        assert r.returncode == 2 and "usage:" in r.stderr, (bad, r.returncode, r.stderr[:200])
    r = subprocess.run([EXE, "--batch", os.path.dirname(glb), "--out", str(tmp_path), *ok, "--score", "2", "--lod-ply", cut], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and "usage:" in r.stderr
    assert not os.path.exists(cut)
