"""-m gpu: the point light baked into spherical harmonics (m2s_bake_light, m2s_sh_shade_records, m2s_export_ply_sh, --bake-light)
against the float64 restatement of tests/bake_ref.py.  Every test prints the figures it asserts on."""
import os
import subprocess

import numpy as np
import pytest

import bake_ref as br
import camera
import light_ref as lr
from mesh2splat_amd import _lib, bake as bk, gltf_io, synth
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prepass import PrepassParams

pytestmark = pytest.mark.gpu
S = 64
SIZES = (1, 63, 64, 65, 257, 1000)
MODEL = camera.trs(translate=(0.2, -0.1, 0.3), rot_axis=(1, 2, 3), rot_deg=35.0, scale=(1.2, 1.2, 0.9))
# the light sits exactly on the float32 world position of the planted record (bake_ref.AT_LIGHT_MODEL)
LIGHT_POS = tuple(float(v) for v in br.world_positions(np.array([br.AT_LIGHT_MODEL + (1.0,) + (0.0,) * 20], np.float32), MODEL)[0])
LIGHT = lr.Light(pos=LIGHT_POS, color=(1.0, 0.9, 0.8), intensity=6.0, far=50.0)
CAM = (0.4, 0.3, 3.5)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def light_params(light=LIGHT):
    return LightParams(light.light_position, light.light_color, light.light_intensity, CAM, light.near_plane, light.far_plane, 6, (64, 64), S, False)


_cases = {}


def case(n):
    """records, cube and the restatement of one size: computed once, shared, never modified"""
    if n not in _cases:
        rec, hostile = br.random_records(n, 100 + n, MODEL, LIGHT)
        cube = br.cube_for(S, 7, LIGHT, LIGHT.far_plane)
        ref, counts = br.bake(rec, MODEL, LIGHT, cube)
        for a in (rec, cube, ref, counts):
            a.setflags(write=False)
        _cases[n] = (rec, hostile, cube, ref, counts)
    return _cases[n]


def check_plane(got, ref, hostile, what):
    """non-finite where (and only where) the restatement is, there at most the hostile records; the rest inside the bar.  -> max |err|"""
    bad_ref, bad_got = ~np.isfinite(ref), ~np.isfinite(got)
    assert np.array_equal(bad_ref, bad_got), f"{what}: non-finite coefficients differ"
    rows = np.flatnonzero(bad_ref.any(-1))
    assert set(rows.tolist()) <= set(hostile), (what, rows)
    fin = ~bad_ref.any(-1)
    if not fin.any():
        return 0.0
    ok, err, tol = br.within_bar(got[fin], ref[fin])
    worst = int(np.argmax(err / tol))
    print(f"{what}: {int(fin.sum())} finite records, max |gpu - ref| {err.max():.3e}, worst err / bar {err[worst] / tol[worst]:.3f} "
          f"(err {err[worst]:.3e}, bar {tol[worst]:.3e})")
    assert ok.all(), f"{what}: {int((~ok).sum())} records outside 1e-4 max|ref| + 1e-6; worst err {err[worst]:.3e} bar {tol[worst]:.3e}"
    assert err.max() <= br.GUARD["sh"], (what, err.max(), br.GUARD["sh"])
    return float(err.max())


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_hostile_records(conv, n):
    rec, hostile, cube, ref, counts = case(n)
    conv.upload_records(rec)
    conv.upload_shadow_cubemap(cube)
    sh, got_counts = conv.bake_light(BakeParams(MODEL, want_shadow_counts=True), light_params())
    assert sh.shape == (n, 48) and sh.dtype == np.float32
    print(f"n = {n}: shadow counts {np.bincount(counts, minlength=21).tolist()}")
    assert np.array_equal(got_counts, counts)
    if n >= 63:                                                                  # both shadowed and lit taps occur
        assert counts.max() > 0 and counts.min() < 20 and len(set(counts.tolist())) > 3
    check_plane(sh, ref, hostile, f"n = {n}")
    if n >= 16:
        assert not np.isfinite(sh[0]).any() and not np.isfinite(sh[1]).any() and not np.isfinite(sh[2]).any()
        assert np.isfinite(sh[3:9]).all()


@pytest.mark.parametrize("nt,nphi", [(4, 8), (4, 16), (8, 8)])
def test_other_tables_and_viewer_metallic(conv, nt, nphi):
    rec, hostile, cube, _, _ = case(257)
    conv.upload_records(rec)
    conv.upload_shadow_cubemap(cube)
    sh = conv.bake_light(BakeParams(MODEL, n_theta=nt, n_phi=nphi, viewer_metallic=True), light_params())
    ref, _ = br.bake(rec, MODEL, LIGHT, cube, n_theta=nt, n_phi=nphi, viewer_metallic=True)
    check_plane(sh, ref, hostile, f"table {nt} x {nphi}, viewer metallic")


def test_intensity_zero_is_flat(conv):
    rec, hostile, cube, _, _ = case(257)
    dark = lr.Light(pos=LIGHT_POS, intensity=0.0, far=50.0)
    conv.upload_records(rec)
    conv.upload_shadow_cubemap(cube)
    sh = conv.bake_light(BakeParams(MODEL), light_params(dark))
    ref, _ = br.bake(rec, MODEL, dark, cube)
    check_plane(sh, ref, hostile, "intensity 0")
    fin = np.isfinite(sh).all(-1)
    a = np.fmin(np.fmax(rec[fin, 4:7], 0), 1).astype(np.float64) ** np.float64(np.float32(2.2))
    c = np.float64(np.float32(0.3)) * a
    f_dc = ((c / (c + 1.0)) ** (1.0 / np.float64(np.float32(2.2))) - 0.5) / bk.C0
    err_dc, rest = np.abs(sh[fin, :3] - f_dc).max(), np.abs(sh[fin, 3:]).max()
    print(f"intensity 0: max |f_dc - (tone - 0.5) / C0| {err_dc:.3e}, max |f_rest| {rest:.3e}")
    assert (np.abs(sh[fin, :3] - f_dc) <= 1e-4 * np.abs(f_dc).max(-1, keepdims=True) + 1e-6).all()
    assert rest <= br.GUARD["sh"]


def test_degrees_pointer_determinism_and_no_shadows(conv):
    import torch
    rec, _, cube, _, _ = case(257)
    conv.upload_records(rec)
    conv.upload_shadow_cubemap(cube)
    lp = light_params()
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    full = conv.bake_light(BakeParams(MODEL, degree=3), lp)
    again = conv.bake_light(BakeParams(MODEL, degree=3), lp)
    assert np.array_equal(bits(full), bits(again))
    for degree in (0, 1, 2):
        want = full.copy().reshape(-1, 48)
        keep = (degree + 1) ** 2
        for c in range(3):
            want[:, 3 + 15 * c + keep - 1:3 + 15 * (c + 1)] = 0.0
        got = conv.bake_light(BakeParams(MODEL, degree=degree), lp)
        assert np.array_equal(bits(got), bits(want)), f"degree {degree}"
    dev = torch.from_numpy(rec.copy()).cuda()
    torch.cuda.synchronize()
    by_pointer = conv.bake_light(BakeParams(MODEL), lp, records=dev)
    assert np.array_equal(bits(by_pointer), bits(full))
    # use_shadows = 0 == a cube that shadows nothing
    conv.upload_shadow_cubemap(np.ones((6, S, S), np.float32))
    lit, counts = conv.bake_light(BakeParams(MODEL, want_shadow_counts=True), lp)
    assert not counts.any()
    unshadowed = conv.bake_light(BakeParams(MODEL, use_shadows=False), lp)
    assert np.array_equal(bits(lit), bits(unshadowed)) and not np.array_equal(bits(lit), bits(full))


def test_sh_shade_records(conv):
    import torch
    rec, hostile, cube, _, _ = case(257)
    conv.upload_records(rec)
    conv.upload_shadow_cubemap(cube)
    sh = conv.bake_light(BakeParams(MODEL), light_params())
    out = conv.sh_shade_records(MODEL, CAM)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = br.shade(rec, sh, MODEL, CAM)
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    others = [k for k in range(24) if k not in (4, 5, 6)]
    assert np.array_equal(u(got)[:, others], u(rec)[:, others])
    bad_ref = ~np.isfinite(ref[:, 4:7])
    assert np.array_equal(bad_ref, ~np.isfinite(got[:, 4:7])) and set(np.flatnonzero(bad_ref.any(-1)).tolist()) <= set(hostile)
    fin = ~bad_ref.any(-1)
    ok, err, tol = br.within_bar(got[fin, 4:7], ref[fin, 4:7])
    print(f"sh_shade: {int(fin.sum())} finite records, max |gpu - ref| {err.max():.3e}, worst err / bar {(err / tol).max():.3f}")
    assert ok.all() and (got[fin, 4:7] >= 0).all()
    assert err.max() <= br.GUARD["shade"]
    # the same through a pointer, into a caller's tensor
    dev = torch.from_numpy(rec.copy()).cuda()
    dst = torch.empty_like(dev)
    torch.cuda.synchronize()
    conv.sh_shade_records(MODEL, CAM, records=dev, out=dst)
    again = dst.cpu().numpy()
    assert ((u(again) == u(got)) | (np.isnan(again) & np.isnan(got))).all()


def test_errors(hiplib):
    import ctypes as C
    from mesh2splat_amd import light as li
    c = Converter(0)
    lc = li.to_c(light_params())
    call = lambda p: c._L.m2s_bake_light(c._h, C.byref(bk.to_c(p)), C.byref(lc), None, 0)
    assert call(BakeParams(MODEL)) == 7                                         # no records
    rec, _, cube, _, _ = case(63)
    c.upload_records(rec)
    assert call(BakeParams(MODEL)) == 7                                         # use_shadows without a cube
    assert call(BakeParams(MODEL, use_shadows=False)) == 0
    c.upload_shadow_cubemap(cube)
    assert call(BakeParams(MODEL, degree=4)) == 1
    assert call(BakeParams(MODEL, n_theta=6)) == 1 and call(BakeParams(MODEL, n_phi=4)) == 1
    bad = bk.to_c(BakeParams(MODEL))
    bad.reserved = 1
    assert c._L.m2s_bake_light(c._h, C.byref(bad), C.byref(lc), None, 0) == 1
    assert call(BakeParams(MODEL)) == 0
    assert c._L.m2s_export_ply_sh(c._h, b"/tmp/never.ply", C.c_float(0.65)) == 7   # uploaded records carry no resolutionTarget
    c.close()


# ---- a converted scene: export, command line, end to end ------------------------------------------------------------------------
R, W, H = 64, 128, 128


def test_export_cli_and_score(conv, tmp_path):
    scene = synth.cube_sphere(6)
    glb = str(tmp_path / "s.glb")
    gltf_io.write_glb(scene, glb)
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
    cli, plain = str(tmp_path / "cli.ply"), str(tmp_path / "plain.ply")
    r = subprocess.run([exe, glb, cli, "--density", str(R), "--bake-light", "--bake-degree", "2", "--light", "1.5,2,2.5,9", "--preview-size", f"{W}x{H}"],
                       capture_output=True, text=True)
    r0 = subprocess.run([exe, glb, plain, "--density", str(R)], capture_output=True, text=True)
    assert r.returncode == 0 and r0.returncode == 0, r.stderr + r0.stderr
    for fmt in ("1", "2"):                                                         # only valid with --format 0: a usage error
        assert subprocess.run([exe, glb, cli + ".no", "--bake-light", "--format", fmt], capture_output=True, text=True).returncode == 2
    kv = dict(p.split("=") for p in [ln for ln in r.stdout.splitlines() if ln.startswith("bake light:")][0].split(":", 1)[1].split())
    near, far = float(kv["near"]), float(kv["far"])
    loaded = gltf_io.load_glb(glb)
    conv.upload_scene(loaded)
    conv.convert(R)
    n = conv.num_stored
    flat = str(tmp_path / "flat.ply")
    conv.export_ply(flat, 0, 0.65)
    assert open(plain, "rb").read() == open(flat, "rb").read()                      # without the flag: today's file
    eye = (0.0, 0.0, 3.2)
    pp = PrepassParams(view_mat=camera.look_at(eye, (0, 0, 0)), proj_mat=camera.perspective(45.0, W / H, near, far), renderer_resolution=(W, H),
                       near_plane=near, far_plane=far, resolution_target=R)
    lp = LightParams((1.5, 2.0, 2.5), (1.0, 1.0, 1.0), 9.0, eye, near, far, 6, (W, H), 1024, False)
    conv.shadow(pp, lp, download=False)
    sh = conv.bake_light(BakeParams(degree=2), lp)
    py = str(tmp_path / "py.ply")
    conv.export_ply_sh(py, 0.65)
    assert open(cli, "rb").read() == open(py, "rb").read()                          # --bake-light == the Python path
    # ... == the host writer over the downloaded records and plane
    import ctypes as C
    rec = conv.download()
    host = str(tmp_path / "host.ply")
    assert conv._L.m2s_write_ply_sh(os.fsencode(host), rec.ctypes.data, sh.ctypes.data, n, C.c_float(np.float32(0.65) / np.float32(R))) == 0
    assert open(host, "rb").read() == open(py, "rb").read() and open(py, "rb").read() != open(flat, "rb").read()
    assert np.isfinite(sh).all() and sh[:, 3:].any()
    # end to end: what a standard viewer shows of the bake against the viewer's own lit frame.  viewer_metallic: that frame's shader reads
    # metallic 0 whatever the records hold (0.1 here: F0 0.097 instead of 0.04, a highlight 2.4 times the frame's)
    mse = {}
    for degree in (0, 3):
        conv.shadow(pp, lp, download=False)
        conv.bake_light(BakeParams(degree=degree, viewer_metallic=True), lp, download=False)
        res = conv.score_baked(pp, lp)
        assert res.pixels > W * H // 20
        mse[degree] = sum(res.sse) / (3.0 * res.pixels)
        print(f"score_baked degree {degree}: {res.pixels} pixels, mean squared error {mse[degree]:.3f} (8-bit units), psnr {res.psnr:.2f} dB")
    assert mse[3] <= mse[0]
