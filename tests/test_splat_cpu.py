"""CPU: the splat pass's ABI mirror and known-answer tests of the numpy restatement (tests/splat_ref.py) the GPU tests check against."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import splat_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def q8(v):
    return int(np.rint(np.clip(np.float32(v), 0, 1) * np.float32(255)))


def test_splat_params_layout_matches_header(tmp_path):
    """m2s_splat_params as the C compiler lays it out == the ctypes mirror in mesh2splat_amd/splat.py."""
    from mesh2splat_amd.splat import SplatParamsC
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = [f[0] for f in SplatParamsC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(m2s_splat_params));\n' +
                   "".join('printf("%%zu\\n", offsetof(m2s_splat_params, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == C.sizeof(SplatParamsC) == 16
    assert [int(v) for v in out[1:]] == [getattr(SplatParamsC, f).offset for f in fields]


def test_centred_gaussian_gives_premultiplied_colour():
    W, H = 64, 32
    q = sr.quad_at(W, H, 10, 7, 3.0, rgb=(0.8, 0.4, 0.2), a=0.75)
    planes, skipped = sr.render(q[None], W, H, 0)
    assert skipped == 0
    alb = planes[2][7, 10]
    f = np.float32
    assert alb.tolist() == [q8(f(0.8) * f(0.75)), q8(f(0.4) * f(0.75)), q8(f(0.2) * f(0.75)), q8(0.75)]
    assert planes[0][7, 10].astype(np.float32).tolist() == [np.float16(v) for v in (1.0, -2.0, 0.5, 1.0)]
    assert planes[4][7, 10].tolist() == [q8(0.25), q8(0.5), 0, 255]
    # a pixel outside the quad stays cleared
    assert not planes[2][0, 0].any() and not planes[0][0, 0].any()


def test_two_centred_gaussians_under_blend():
    """Front quad (array order 0) then back quad: closed form of ONE_MINUS_DST_ALPHA / ONE with the RGBA8 quantisation."""
    W, H = 64, 32
    front = sr.quad_at(W, H, 20, 10, 2.0, rgb=(1.0, 0.0, 0.0), a=0.5)
    back = sr.quad_at(W, H, 20, 10, 2.0, rgb=(0.0, 1.0, 0.0), a=0.5)
    planes, _ = sr.render(np.stack([front, back]), W, H, 0)
    f = np.float32
    a1 = f(q8(0.5)) / f(255)                     # 128 / 255 read back
    t = f(1) - a1
    assert planes[2][10, 20].tolist() == [q8(f(0) * t + a1), q8(f(0.5) * t + f(0)), 0, q8(f(0.5) * t + a1)]
    # position alpha: g = 1, then 1 * (1 - 1) + 1
    assert planes[0][10, 20, 3] == np.float16(1.0)


def test_shared_edge_covers_each_centre_once():
    """Two quads sharing an edge through a column of pixel centres: every centre on it gets exactly one fragment (mode 4: G = count)."""
    W, H = 32, 32
    left = np.zeros(24, np.float32)
    right = np.zeros(24, np.float32)
    # left quad spans x in [4, 16] px, right quad [16, 28] px; the shared edge x = 16 px sits on... pixel centres are at +0.5,
    # so shift by half a pixel: edges at 4.5, 16.5, 28.5 (centres of columns 4, 16, 28)
    for qq, (xa, xb) in ((left, (4.5, 16.5)), (right, (16.5, 28.5))):
        cx, hx = (xa + xb) / 2, (xb - xa) / 2
        qq[0] = cx / (W / 2) - 1
        qq[1] = 16.0 / (H / 2) - 1
        qq[4] = hx / (W / 2)
        qq[7] = 8.5 / (H / 2)
        qq[11] = 1.0
        qq[12], qq[14] = 0.01, 0.01
    planes, _ = sr.render(np.stack([left, right]), W, H, 4)
    g = planes[2][:, :, 1]
    rows = slice(8, 24)
    assert (g[rows, 16] == 1).all()           # min(k, 255) with k = 1 on the shared column
    assert (g[rows, 5:16] == 1).all() and (g[rows, 17:28] == 1).all()


def test_overdraw_counts_fragments():
    W, H = 16, 16
    q = sr.quad_at(W, H, 8, 8, 3.0)
    for k in (1, 2, 5, 90, 100):
        planes, _ = sr.render(np.repeat(q[None], k, 0), W, H, 4)
        assert planes[2][8, 8].tolist() == [min(3 * k, 255), min(k, 255), 0, min(3 * k, 255)]


def test_skips_non_finite_and_far_quads():
    W, H = 16, 16
    q = np.repeat(sr.quad_at(W, H, 8, 8, 3.0)[None], 4, 0)
    q[1, 13] = np.nan                          # conic.y
    q[2, 4] = 1e4                              # an axis far beyond the guard band
    q[3, 2] = np.inf                           # mean.z is not read
    planes, skipped = sr.render(q, W, H, 4)
    assert skipped == 2 and planes[2][8, 8, 1] == 2


def test_restatement_is_not_imported_by_the_product():
    import re
    for dp, _, files in os.walk(os.path.join(ROOT, "mesh2splat_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert not re.search(r"^\s*(from|import)\s+\S*splat_ref", txt, flags=re.M), f
