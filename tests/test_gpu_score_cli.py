"""-m gpu: `mesh2splat in.glb out.ply --score K`: the JSON record against Converter.score through cameras rebuilt from the printed eyes,
and the error maps of --score-map."""
import json
import os
import subprocess

import numpy as np
import pytest

from mesh2splat_amd import _lib, gltf_io, synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.score import camera_from_eye, orbit_cameras, pool

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
W, H, R, K = 96, 64, 64, 2


def score_line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("score: ")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0][len("score: "):])


def test_cli_score(tmp_path, hiplib):
    import PIL.Image
    glb, out, prefix = str(tmp_path / "s.glb"), str(tmp_path / "s.ply"), str(tmp_path / "err")
    gltf_io.write_glb(synth.sphere_grid(2, n=5, tex_size=32), glb)
    r = subprocess.run([EXE, glb, out, "--density", str(R), "--preview-size", f"{W}x{H}", "--score", str(K), "--score-elevation", "15", "--score-map", prefix],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    rec = score_line(r.stdout)
    assert rec["views"] == K == len(rec["per_view"]) and rec["size"] == [W, H] and rec["mask"] == 2 and rec["mode"] == 6 and rec["density"] == R
    loaded = gltf_io.load_glb(glb)
    # the camera rule: the printed eyes are orbit_cameras' (sin / cos of the same libm; compared to a few ulps, then taken as printed)
    for cam, view in zip(orbit_cameras(loaded, K, W, H, elevation_deg=15.0), rec["per_view"]):
        assert np.allclose(cam.eye, view["eye"], rtol=1e-12, atol=1e-12) and np.allclose(cam.centre, rec["centre"], rtol=1e-15)
        assert np.isclose(cam.near, rec["near"], rtol=1e-14) and np.isclose(cam.far, rec["far"], rtol=1e-14)
    light = rec["light"]
    views = []
    with Converter(0) as conv:
        conv.upload_scene(loaded)
        conv.convert(R)
        for k, view in enumerate(rec["per_view"]):
            cam = camera_from_eye(view["eye"], rec["centre"], rec["near"], rec["far"], W, H)
            got = conv.score(*cam.frame_params(R, light["position"], light["intensity"]), mask_mode=2, want_map=True)
            views.append(got)
            assert got.integers() == {key: view[key] for key in got.integers()}, k
            img = np.asarray(PIL.Image.open(f"{prefix}_{k}.png").convert("RGBA"))
            assert img.shape == (H, W, 4) and np.array_equal(img, got.error_map[::-1])            # top row first
            assert got.pixels > 0 and got.windows > 0
    p = pool(views)
    assert p.integers() == {key: rec["pooled"][key] for key in p.integers()}
    assert rec["pooled"]["psnr_db"] == pytest.approx(p.psnr, rel=1e-12) and rec["pooled"]["ssim"] == pytest.approx(p.ssim, rel=1e-12)
    assert rec["pooled"]["coverage_iou"] == pytest.approx(p.coverage_iou, rel=1e-12)
    assert not os.path.exists(f"{prefix}_{K}.png")


def test_cli_score_beside_a_preview_and_bad_arguments(tmp_path, hiplib):
    glb, out, png = str(tmp_path / "q.glb"), str(tmp_path / "q.ply"), str(tmp_path / "view.png")
    gltf_io.write_glb(synth.unit_quad(synth.procedural_textures(32, 3)), glb)
    base = [EXE, glb, out, "--density", "48", "--preview-size", "64x48"]
    alone = subprocess.run(base + ["--score", "1", "--score-mask", "3", "--preview-mode", "0"], capture_output=True, text=True, timeout=300)
    both = subprocess.run(base + ["--score", "1", "--score-mask", "3", "--preview-mode", "0", "--preview", png], capture_output=True, text=True, timeout=300)
    assert alone.returncode == 0 and both.returncode == 0, alone.stderr + both.stderr
    a, b = score_line(alone.stdout), score_line(both.stdout)
    assert a == b and a["mode"] == 0 and a["mask"] == 3 and os.path.exists(png) and "preview camera:" in both.stdout and "preview camera:" not in alone.stdout
    assert a["per_view"][0]["pixels"] == a["per_view"][0]["cover"][3] > 0
    for bad in (["--score", "0"], ["--score", "1", "--score-mask", "4"], ["--score", "1", "--score-elevation", "90"]):
        assert subprocess.run(base + bad, capture_output=True, text=True, timeout=60).returncode == 2
