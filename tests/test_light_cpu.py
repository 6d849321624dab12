"""CPU: the numpy restatement of the shadow and relighting passes (tests/light_ref.py) against cases worked out by hand, the C layout
of m2s_light_params against its ctypes mirror, and the conditioning cap of the relighting cases the GPU test uses."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import light_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_light_params_layout_matches_header(tmp_path):
    """m2s_light_params / m2s_shadow_quad as the C compiler lays them out == the ctypes mirror in mesh2splat_amd/light.py."""
    from mesh2splat_amd.light import LightParamsC
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = [n for n, _ in LightParamsC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){\n'
                   'printf("%zu %zu\\n", sizeof(m2s_light_params), sizeof(m2s_shadow_quad));\n' +
                   "".join('printf("%%zu\\n", offsetof(m2s_light_params, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert int(out[0]) == C.sizeof(LightParamsC) == 72 and int(out[1]) == 48
    assert [int(v) for v in out[2:]] == [getattr(LightParamsC, f).offset for f in fields]


def test_cube_lookup_one_texel_of_each_face():
    """OpenGL 4.6 table 8.19 by hand, S = 8: s = 0.5 (sc / |ma| + 1), texel floor(8 s)."""
    cube = np.arange(6 * 8 * 8, dtype=np.float32).reshape(6, 8, 8)
    cases = [((1.0, 0.5, -0.25), (0, 2, 5)),     # +X: sc = -z = .25 -> s = .625 -> 5; tc = -y = -.5 -> t = .25 -> 2
             ((-2.0, 1.0, 1.0), (1, 2, 6)),      # -X: sc = z = 1, /2 -> s = .75 -> 6; tc = -y = -1, /2 -> t = .25 -> 2
             ((0.25, 1.0, 0.5), (2, 6, 5)),      # +Y: sc = x = .25 -> s = .625 -> 5; tc = z = .5 -> t = .75 -> 6
             ((0.25, -1.0, 0.5), (3, 2, 5)),     # -Y: sc = x -> 5; tc = -z = -.5 -> t = .25 -> 2
             ((-0.5, 0.75, 1.0), (4, 1, 2)),     # +Z: sc = x = -.5 -> s = .25 -> 2; tc = -y = -.75 -> t = .125 -> 1
             ((-0.5, 0.75, -1.0), (5, 1, 6)),    # -Z: sc = -x = .5 -> s = .75 -> 6; tc = -y -> 1
             ((1.0, 1.0, 1.0), (0, 0, 0)),       # ties go to x, then y: +X, sc = -1 -> s = 0 -> 0, tc = -1 -> 0
             ((0.0, 1.0, 1.0), (2, 7, 4)),       # |y| >= |z|: +Y, sc = 0 -> s = .5 -> 4; tc = z = 1 -> t = 1 -> floor(8) clamped to 7
             ((np.nan, 1.0, 0.0), (5, 0, 0)),    # a NaN coordinate reads texel (0, 0) of face 5
             ((0.0, 0.0, 0.0), (5, 0, 0))]       # 0 / 0
    for v, (face, j, i) in cases:
        got = lr.cube_texel(cube, *(np.array([c], np.float32) for c in v))[0]
        assert got == cube[face, j, i], (v, got, cube[face, j, i])


def test_one_occluder_one_receiver():
    """Light at the origin, an opaque quad of half-size 0.25 NDC on face -Z at distance 1, receiver at z = -3: 20 taps shadowed behind
    the occluder (the widest tap, 0.025 sqrt(2) off axis, stays inside 0.25), none beside it."""
    S, far = 64, 50.0
    lists = [np.zeros((0, 12), np.float32) for _ in range(6)]
    lists[5] = np.array([[0, 0, 0.5, 1, 0.25, 0, 0, -0.25, 0, 0, -1, 1]], np.float32)
    cube, skipped = lr.shadow_cube(lists, S, (0, 0, 0), far)
    assert skipped == 0
    assert (cube[:5] == 1.0).all()
    inside = cube[5] < 1.0
    assert inside.sum() == 16 * 16 and inside[24:40, 24:40].all()           # NDC +-0.25 of 64 texels: 24..39
    assert (cube[5][inside] == f32(1.0) / f32(far)).all()
    pos = np.array([[0, 0, -3], [2.5, 0, -3], [0, 0, -0.9]], np.float32)    # behind, beside, in front of the occluder
    assert lr.shadow_counts(pos, cube, (0, 0, 0), far).tolist() == [20, 0, 0]


def test_stage_a_faces_ties_and_nan():
    """determineFaceIndex's `if` chain: ties go to x, then y; a NaN direction (a record at the light, a NaN position) lands on face 5."""
    rec = np.zeros((5, 24), np.float32)
    rec[:, 3] = 1
    rec[:, 8:11] = 0.01
    rec[:, 16] = 1                                  # identity rotation
    rec[0, 0:3] = (1, 1, 0)                         # |x| = |y|: face 0
    rec[1, 0:3] = (0, -1, -1)                       # |y| = |z|: face 3
    rec[2, 0:3] = (0, 0, 0)                         # at the light: 0 / 0
    rec[3, 0:3] = (np.nan, 0, 1)
    rec[4, 0:3] = (0.1, 0.2, 2)                     # face 4
    lists = lr.shadow_quads(rec, np.eye(4, dtype=np.float32), (64, 64), (0.01, 50.0), 1.0, 1, 0, (0, 0, 0), (0.01, 50.0))
    n = [q.shape[0] for q in lists]
    assert n[0] == 1 and n[3] == 1 and n[4] == 1 and n[1] == n[2] == 0
    # the NaN position is kept (no comparison culls a NaN), on face 5; the record AT the light goes to face 5 too and is culled there
    # by the tests that follow, as written: w = 0 and z = -2 f n / (f - n) < -1.05 w
    assert n[5] == 1 and np.isnan(lists[5]).any(1).all()
    # +X camera: x_view = -z, y_view = -y, depth x: the record at (1, 1, 0) projects to NDC (0, -1)
    assert lists[0][0, 0] == 0 and lists[0][0, 1] == -1 and lists[0][0, 8:11].tolist() == [1, 1, 0]
    # 3 sigma = 0.03 at distance 2 with a 64 px window: 32 px per unit / 2 -> sigma 0.16 px; +0.3 low-pass -> 3 sqrt(0.3256) px / 32
    assert abs(float(lists[4][0, 4:6].dot(lists[4][0, 4:6])) ** 0.5 - 3 * (0.16 ** 2 + 0.3) ** 0.5 / 32) < 1e-3


def test_pi_macro_expansion_on_one_pixel():
    """N = L = V = H = +z, roughness 1, albedo 1, light colour x intensity / d^2 = 1: every dot product is 1, NDF = 1 / ((22/7) 1 1),
    G = 1, F = 0.04, kD = 0.96; `kD * albedo / PI` expands to ((0.96) / 22) / 7 — not 0.96 / (22 / 7)."""
    pos = np.zeros((1, 1, 4), np.float16)
    nrm = np.array([[[0.5, 0.5, 1.0, 1.0]]], np.float16)
    alb = np.full((1, 1, 4), 255, np.uint8)
    mr = np.array([[[0, 255, 0, 255]]], np.uint8)
    lp = lr.Light(pos=(0, 0, 2), color=(1, 1, 1), intensity=4.0, cam=(0, 0, 2), far=50.0)
    cube = np.ones((6, 4, 4), np.float32)
    frame, counts, ill = lr.relight([pos, nrm, alb, np.zeros((1, 1, 4), np.float16), mr], cube, lp)
    assert counts[0, 0] == 0 and not ill[0, 0]
    spec = ((7.0 / 22.0) * 1.0 * 0.04) / (4.0 + 0.0001)
    col = 0.3 + ((0.96 / 22.0) / 7.0 + spec) * 1.0
    want = round(min(max((col / (col + 1.0)) ** (1 / 2.2), 0), 1) * 255)
    wrong = 0.3 + (0.96 / (22.0 / 7.0) + spec)
    assert want != round((wrong / (wrong + 1.0)) ** (1 / 2.2) * 255)        # the two readings of the macro differ on this pixel
    assert frame[0, 0].tolist() == [want, want, want, 255]
    for mode, src in ((0, alb), (5, mr)):
        f, _, _ = lr.relight([pos, nrm, alb, None, mr], cube, lp, mode)
        assert f[0, 0].tolist() == ([255, 255, 255, 255] if mode == 0 else [0, 255, 0, 255])


@pytest.mark.parametrize("case", lr.RELIGHT_CASES)
def test_ill_conditioned_share_of_the_gpu_cases(case):
    """The GPU test exempts ill-conditioned pixels from the 1 LSB bound; they must be at most 0.5 % of each of its cases."""
    lp = lr.Light()
    planes = lr.random_gbuffer(case["W"], case["H"], case["seed"], case["edge"])
    cube = lr.random_cube(case["S"], case["seed"], lp.far_plane)
    _, counts, ill = lr.relight(planes, cube, lp)
    print(f"case {case}: ill-conditioned share {ill.mean():.5f}, counts 0 / 1..19 / 20: {(counts == 0).mean():.3f} / "
          f"{((counts > 0) & (counts < 20)).mean():.3f} / {(counts == 20).mean():.3f}")
    assert ill.mean() <= lr.ILL_SHARE_MAX
    assert ((counts > 0) & (counts < 20)).any()
