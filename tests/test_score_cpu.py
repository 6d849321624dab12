"""CPU: the numpy restatement of the fidelity score (tests/score_ref.py) against cases worked out by hand, the C layout of
m2s_score_params / m2s_score_result against their ctypes mirrors, the ratios the binding derives, and the cameras of --score."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import camera
import score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_structs_layout_matches_header(tmp_path):
    """m2s_score_params / m2s_score_result as the C compiler lays them out: 24 and 120 bytes, == the ctypes mirrors."""
    from mesh2splat_amd.score import ScoreParamsC, ScoreResultC
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    pf, rf = [n for n, _ in ScoreParamsC._fields_], [n for n, _ in ScoreResultC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){\n'
                   'printf("%zu %zu %d\\n", sizeof(m2s_score_params), sizeof(m2s_score_result), M2S_ABI_VERSION);\n' +
                   "".join('printf("%%zu\\n", offsetof(m2s_score_params, %s));\n' % f for f in pf) +
                   "".join('printf("%%zu\\n", offsetof(m2s_score_result, %s));\n' % f for f in rf) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert out[0] == C.sizeof(ScoreParamsC) == 24 and out[1] == C.sizeof(ScoreResultC) == 120 and out[2] == 1
    assert out[3:3 + len(pf)] == [getattr(ScoreParamsC, f).offset for f in pf]
    assert out[3 + len(pf):] == [getattr(ScoreResultC, f).offset for f in rf]


def test_identical_8x8_images():
    img = np.random.default_rng(1).integers(0, 256, (8, 8, 4), dtype=np.uint8)
    r = sr.score(img, img.copy(), flags=sr.NO_COVER)
    assert r["windows"] == 1 and r["ssim_q32"] == 2 ** 32 and r["sse"] == [0, 0, 0] and r["sad"] == [0, 0, 0] and r["max_abs"] == [0, 0, 0]
    assert r["pixels"] == 64 and r["cover"] == [0, 0, 0, 64]
    assert math.isinf(sr.psnr(r))


def test_black_against_white_8x8():
    a, b = np.zeros((8, 8, 4), np.uint8), np.full((8, 8, 4), 255, np.uint8)
    q, (s1, s2, ssq, s12) = sr.window_q(sr.luma(a), sr.luma(b))
    assert (s1, s2, ssq, s12) == (0, 16320, 4161600, 0)
    r = sr.score(a, b, flags=sr.NO_COVER)
    assert r["sse"] == [64 * 65025] * 3 and r["sad"] == [64 * 255] * 3 and r["max_abs"] == [255] * 3 and r["windows"] == 1
    exact = Fraction(26634 * 2 ** 32, 266369034)          # num / den = c1 c2 / ((s2^2 + c1) c2): the rational, independent of fp64
    assert abs(r["ssim_q32"] - round(exact)) <= 1 and r["ssim_q32"] == q
    assert abs(sr.psnr(r)) < 1e-12                        # 10 log10(255^2 * 3 * 64 / (3 * 64 * 255^2)) = 0 dB


def test_luma_weights():
    assert 77 + 150 + 29 == 256
    assert sr.luma(np.array([[[255, 255, 255, 0]]], np.uint8))[0, 0] == 255 and sr.luma(np.zeros((1, 1, 4), np.uint8))[0, 0] == 0
    assert sr.luma(np.array([[[255, 0, 0, 9]]], np.uint8))[0, 0] == (77 * 255 + 128) >> 8


def test_mask_rule_31_and_32():
    rng = np.random.default_rng(2)
    a, b = (rng.integers(0, 256, (8, 8, 4), dtype=np.uint8) for _ in range(2))
    cb = np.zeros((8, 8, 4), np.uint8)
    for n, counted in ((31, 0), (32, 1)):
        ca = np.zeros((64, 4), np.uint8)
        ca[rng.permutation(64)[:n], 3] = rng.integers(1, 256, n)
        r = sr.score(a, b, ca.reshape(8, 8, 4), cb, mask_mode=1)
        assert r["pixels"] == n and r["windows"] == counted and r["cover"] == [64 - n, n, 0, 0]
        # all 64 pixels enter a counted window's sums: the same q as without a mask
        assert r["ssim_q32"] == (sr.score(a, b, flags=sr.NO_COVER)["ssim_q32"] if counted else 0)
    r3 = sr.score(a, b, ca.reshape(8, 8, 4), cb, mask_mode=3)
    assert r3["pixels"] == 0 and r3["sse"] == [0, 0, 0] and math.isnan(sr.psnr(r3))


def test_windows_of_a_ragged_image_and_the_map():
    rng = np.random.default_rng(3)
    a, b, ca, cb = (rng.integers(0, 256, (13, 18, 4), dtype=np.uint8) for _ in range(4))
    r = sr.score(a, b, ca, cb, mask_mode=0, flags=sr.WANT_MAP)
    assert r["windows"] == 2 * 3                          # origins x = 0, 4, 8 (8 + 8 <= 18), y = 0, 4 (4 + 8 <= 13)
    assert r["pixels"] == 13 * 18 and sum(r["cover"]) == 13 * 18
    assert (r["map"][..., 3] == 255).all() and int(r["map"][..., :3].astype(np.int64).sum()) == sum(r["sad"])
    assert sr.score(a[:7], b[:7], flags=sr.NO_COVER)["windows"] == 0


def test_binding_ratios():
    from mesh2splat_amd.score import ScoreResult, pool
    r = ScoreResult(pixels=100, cover=(10, 20, 30, 50), sse=(100, 200, 0), sad=(10, 20, 0), max_abs=(3, 4, 0), windows=4, ssim_q32=3 * 2 ** 32)
    assert r.ssim == 0.75 and r.coverage_iou == 0.5 and abs(r.psnr - 10 * math.log10(65025 * 3 * 100 / 300)) < 1e-12
    empty = ScoreResult()
    assert math.isnan(empty.psnr) and math.isnan(empty.ssim) and math.isnan(empty.coverage_iou)
    assert math.isinf(ScoreResult(pixels=5).psnr)
    p = pool([r, ScoreResult(pixels=1, cover=(0, 0, 0, 1), sse=(1, 1, 1), sad=(1, 1, 1), max_abs=(1, 9, 1), windows=0, ssim_q32=0)])
    assert p.pixels == 101 and p.cover == (10, 20, 30, 51) and p.sse == (101, 201, 1) and p.max_abs == (3, 9, 1) and p.windows == 4
    assert p.ssim == 0.75


def test_orbit_cameras_view_0_is_the_preview_camera():
    from mesh2splat_amd import synth
    from mesh2splat_amd.score import orbit_cameras, preview_rule
    scene = synth.sphere_grid(2, n=5, tex_size=8)
    W, H = 160, 100
    mn = np.min([m.bbox_min for m in scene.meshes], 0).astype(np.float64)
    mx = np.max([m.bbox_max for m in scene.meshes], 0).astype(np.float64)
    ctr = (mn + mx) / 2
    radius = math.sqrt(sum((mx[k] - mn[k]) * (mx[k] - mn[k]) for k in range(3))) / 2
    dist = 1.1 * radius / math.tan(22.5 * (math.pi / 180.0))
    cam, = orbit_cameras(scene, 1, W, H)
    assert cam.eye == (ctr[0], ctr[1], ctr[2] + dist) and cam.centre == tuple(ctr) and cam.near == dist / 100 and cam.far == dist * 10
    assert np.array_equal(cam.view_mat, camera.look_at(cam.eye, cam.centre))
    assert np.array_equal(cam.proj_mat, camera.perspective(45.0, W / H, cam.near, cam.far))
    assert preview_rule((mn, mx)) == preview_rule(scene)
    # K views: on the circle round the centre, half a turn apart for K = 2; the elevation raises the eye
    c0, c1 = orbit_cameras((mn, mx), 2, W, H)
    assert c0.eye == cam.eye and np.allclose(c1.eye, (ctr[0], ctr[1], ctr[2] - dist))
    up, = orbit_cameras(scene, 1, W, H, elevation_deg=30.0)
    assert np.isclose(up.eye[1] - ctr[1], dist / 2) and np.isclose(np.linalg.norm(np.subtract(up.eye, ctr)), dist)
    with pytest.raises(ValueError):
        orbit_cameras(scene, 1, W, H, elevation_deg=90.0)
