"""-m gpu: the splat pass (m2s_splat, k_splat_*) through the C ABI against the numpy restatement tests/splat_ref.py.
Exact = byte-identical.  Mode 4 (overdraw) pins coverage and order: its albedo G channel is the per-pixel fragment count and its
blend has no exp in the albedo plane.  Pixel-centre Gaussians (g = exp(0) = 1 whatever exp is used) pin the blend of every other
mode exactly; elsewhere the device's fast exp may move values by a few LSB, within the bounds below."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import splat_ref as sr
from mesh2splat_amd import _lib, synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.splat import SplatParams

pytestmark = pytest.mark.gpu
U8_TOL = 1            # unorm8 LSB (measured: 1)
F16_REL = 2e-3        # fp16: |got - want| <= F16_REL * max(1, |want|) (measured: 1.03e-3, one half ulp at 1)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def run(conv, quads, W, H, mode):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(quads, np.float32).reshape(-1, 24)).cuda()
    planes, skipped = conv.splat(SplatParams((W, H), mode), quads=t)
    return planes, skipped


def assert_exact(got, want, what, planes=range(5)):
    for k in planes:
        g, w = got[k], want[k]
        if g.dtype == np.float16:
            ok = g.view(np.uint16) == w.view(np.uint16)
        else:
            ok = g == w
        assert ok.all(), f"{what}: attachment {k} differs at {np.argwhere(~ok.all(-1))[:5].tolist()} got {g[~ok.all(-1)][:3].tolist()} want {w[~ok.all(-1)][:3].tolist()}"


def max_diffs(got, want):
    """-> (max unorm8 |d| over attachments 2 and 4, max fp16 |d| / max(1, |want|) over 0, 1, 3); +-0 are equal"""
    d8 = max(int(np.abs(got[k].astype(np.int32) - want[k].astype(np.int32)).max(initial=0)) for k in (2, 4))
    dh = 0.0
    for k in (0, 1, 3):
        g, w = got[k].astype(np.float64), want[k].astype(np.float64)
        both = np.isfinite(g) & np.isfinite(w)
        assert ((np.isnan(g) == np.isnan(w)) & (np.isinf(g) == np.isinf(w))).all(), f"attachment {k}: non-finite values differ"
        r = np.abs(g - w)[both] / np.maximum(1.0, np.abs(w[both]))
        dh = max(dh, float(r.max(initial=0.0)))
    return d8, dh


def assert_close(got, want, what):
    d8, dh = max_diffs(got, want)
    print(f"{what}: max unorm8 |d| = {d8} LSB, max fp16 rel |d| = {dh:.3g}")
    assert d8 <= U8_TOL and dh <= F16_REL, (what, d8, dh)


# ---- coverage and order, exact (mode 4) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n,seed", [(641, 359, 3000, 1), (1, 1, 50, 2), (64, 48, 500, 3)])
def test_overdraw_random_quads_exact(conv, W, H, n, seed):
    q = sr.random_quads(n, W, H, seed, max_px=40.0)
    got, sk = run(conv, q, W, H, 4)
    want, wsk = sr.render(q, W, H, 4)
    assert sk == wsk == 0
    assert_exact(got, want, f"overdraw {W}x{H}", planes=(2,))
    assert got[2][..., 1].max() > 1           # overlaps exist


def test_overdraw_tile_borders_offscreen_pixel_edges_zero_area(conv):
    W, H = 100, 70
    qs = []
    # quads exactly on pixel-centre edges (the top-left rule decides), across tile borders, partly off screen
    for (cx, cy, hx, hy) in ((16.0, 16.0, 4.0, 4.0), (15.5, 31.5, 8.0, 8.0), (0.0, 0.0, 10.0, 6.0), (99.5, 69.5, 12.0, 3.0),
                             (48.0, 32.0, 16.0, 16.0), (33.5, 47.5, 0.5, 9.0), (60.0, 10.0, 0.0, 5.0), (70.0, 20.0, 0.0, 0.0)):
        q = np.zeros(24, np.float32)
        q[0], q[1] = cx / (W / 2) - 1, cy / (H / 2) - 1
        q[4], q[7] = hx / (W / 2), hy / (H / 2)
        q[11], q[12], q[14] = 0.9, 0.02, 0.02
        qs.append(q)
    # rotated (sheared) quad sharing its diagonal through pixel centres
    q = np.zeros(24, np.float32)
    q[0], q[1] = 40.5 / (W / 2) - 1, 40.5 / (H / 2) - 1
    q[4], q[5], q[6], q[7] = 8 / (W / 2), 8 / (H / 2), -8 / (W / 2), 8 / (H / 2)
    q[11], q[12], q[14] = 1.0, 0.02, 0.02
    qs.append(q)
    qs = np.stack(qs)
    got, _ = run(conv, qs, W, H, 4)
    want, _ = sr.render(qs, W, H, 4)
    assert_exact(got, want, "edges", planes=(2,))


def test_overdraw_nan_and_guard_band_skipped(conv):
    W, H = 128, 96
    q = sr.random_quads(400, W, H, 7)
    q[5, 13] = np.nan
    q[17, 0] = np.inf
    q[33, 4] = 1e5
    q[40, 22] = -np.inf
    q[41, 2] = np.nan                      # mean.z is not read: drawn
    got, sk = run(conv, q, W, H, 4)
    want, wsk = sr.render(q, W, H, 4)
    assert sk == wsk == 4
    assert_exact(got, want, "skips", planes=(2,))
    assert conv.last_splat_counts()["skipped"] == 4


def test_overdraw_one_tile_many_batches(conv):
    """A single tile with more quads than one LDS batch (256), in an order that matters for nothing but the count."""
    W, H = 16, 16
    q = sr.random_quads(1000, W, H, 11, max_px=12.0)
    q[:, 0] = np.clip(q[:, 0], -0.9, 0.9)
    q[:, 1] = np.clip(q[:, 1], -0.9, 0.9)
    got, _ = run(conv, q, W, H, 4)
    want, _ = sr.render(q, W, H, 4)
    assert_exact(got, want, "one tile", planes=(2,))
    assert conv.last_splat_counts()["pairs"] == 1000


# ---- pixel-centre KATs, exact in modes 0 and 5 --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 5])
def test_pixel_centre_kats_exact(conv, mode):
    W, H = 64, 32
    qs = [sr.quad_at(W, H, 20, 10, 2.0, rgb=(0.9, 0.3, 0.1), a=0.6, ws=(1.5, -2.25, 0.125), normal=(0.0, -0.6, 0.8), depth=7.5),
          sr.quad_at(W, H, 20, 10, 1.0, rgb=(0.2, 0.7, 0.4), a=0.45, ws=(-3.0, 0.5, 2.0), normal=(1.0, 0.0, 0.0), depth=2.25,
                     metallic=0.9, roughness=0.1),
          sr.quad_at(W, H, 20, 10, 3.0, rgb=(0.5, 0.5, 0.9), a=0.3, ws=(0.1, 0.2, 0.3), depth=11.0)]
    qs = np.stack(qs)
    px = (10, 20)
    rev = None
    for order in (qs, qs[::-1].copy()):
        got, _ = run(conv, order, W, H, mode)
        want, _ = sr.render(order, W, H, mode)
        for k in range(5):
            a, b = got[k][px], want[k][px]
            if a.dtype == np.float16:
                assert (a.view(np.uint16) == b.view(np.uint16)).all(), (mode, k, a, b)
            else:
                assert (a == b).all(), (mode, k, a, b)
        if rev is None:
            rev = [p[px].copy() for p in got]
        else:
            assert any(not np.array_equal(rev[k], got[k][px]) for k in range(5)), "reversing the order changed nothing"


# ---- values within tolerance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_random_overlapping_quads_close(conv, mode):
    W, H = 200, 120
    q = sr.random_quads(2500, W, H, 21 + mode, max_px=30.0)
    got, _ = run(conv, q, W, H, mode)
    want, _ = sr.render(q, W, H, mode)
    assert_close(got, want, f"random mode {mode}")


def _frame(conv, scene, R, W, H, eye=(1.6, 1.1, 2.3), target=(0.1, 0.0, -0.1)):
    import camera
    from mesh2splat_amd.prepass import PrepassParams
    conv.upload_scene(scene)
    conv.convert(R)
    pp = PrepassParams(view_mat=camera.look_at(eye, target), proj_mat=camera.perspective(45.0, W / H, 0.01, 100.0),
                       renderer_resolution=(W, H), resolution_target=R)
    conv.prepass(pp, download=False)
    return conv.sort_prepass()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_real_frame_close(conv, mode):
    scene = synth.cube_sphere(40, tex_size=64)
    W, H = 320, 180
    sq = _frame(conv, scene, 128, W, H)
    planes, sk = conv.splat(SplatParams((W, H), mode))
    assert sk == 0
    want, _ = sr.render(sq, W, H, mode)
    assert_close(planes, want, f"frame mode {mode}")
    if mode == 0:
        assert (planes[2][..., 3] > 0).mean() > 0.05
        # the reference-shaped pass on the same context: same planes
        from mesh2splat_amd.converter import GaussianSplattingPass, RenderContext
        ctx = RenderContext(scene)
        ctx.converter, ctx.rendererResolution, ctx.renderMode = conv, (W, H), 0
        GaussianSplattingPass().execute(ctx)
        assert ctx.splatSkipped == 0 and all(np.array_equal(a, b) for a, b in zip(ctx.gBuffer, planes))


def test_saturating_pixel_early_exit_is_exact(conv):
    """Opaque quads centred on one pixel drive all five alphas to exactly 1.0; more quads follow (some with -0 sources and one
    with a degenerate conic, which the early exit must not skip blindly)."""
    W, H = 32, 32
    base = sr.quad_at(W, H, 12, 12, 6.0, rgb=(0.7, 0.2, 0.9), a=1.0, conic=(0.02, 0.0, 0.02), ws=(0.5, -0.25, 2.0))
    qs = [base.copy() for _ in range(12)]
    for k in range(300):
        q = sr.quad_at(W, H, 12, 12, 5.0, rgb=(0.1, 0.9, 0.3), a=0.8, conic=(0.05, 0.01, 0.03), ws=(-1.0, 0.0, -0.0), normal=(-0.0, 1.0, 0.0))
        q[0] += np.float32(1e-3 * (k % 7))
        qs.append(q)
    odd = base.copy()
    odd[12:15] = (-0.01, 0.0, 0.02)           # not positive definite: g > 1 away from the centre
    qs.append(odd)
    qs = np.stack(qs).astype(np.float32)
    got, _ = run(conv, qs, W, H, 0)
    want, _ = sr.render(qs, W, H, 0)
    assert want[0][12, 12, 3] == 1.0 and want[2][12, 12, 3] == 255 and want[4][12, 12, 3] == 255
    assert_exact([g[12:13, 12:13] for g in got], [w[12:13, 12:13] for w in want], "saturated pixel")
    assert_close(got, want, "saturating stack")


# ---- full-size frame ----------------------------------------------------------------------------------------------------------
def test_c3_full_frame(conv):
    import torch
    W, H = 1920, 1080
    scene = synth.cube_sphere(289, tex_size=2048)
    sq = _frame(conv, scene, 1024, W, H)
    assert sq.shape[0] > 100_000
    planes, sk = conv.splat(SplatParams((W, H), 0))
    s = sr.setup(sq, W, H)
    # the prepass's quads never reach the guard band (include/m2s.h); a quad it wrote with a non-finite field is skipped and counted
    bad = np.nonzero(s["skip"])[0]
    print("C3 frame: skipped quads", bad.tolist(), sq[bad].tolist())
    assert sk == bad.size and all(not np.isfinite(np.concatenate([sq[i, 0:2], sq[i, 4:24]])).all() for i in bad)
    again, _ = conv.splat(SplatParams((W, H), 0))
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(planes, again)), "two calls differ"
    explicit, _ = conv.splat(SplatParams((W, H), 0), quads=torch.from_numpy(sq).cuda())
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(planes, explicit)), "NULL path != explicit pointer"
    over, _ = conv.splat(SplatParams((W, H), 4), quads=torch.from_numpy(sq).cuda())
    counts = conv.last_splat_counts()
    print("C3 frame:", sq.shape[0], "quads,", counts)
    tc = sr.tile_counts(s)
    assert int(tc.sum()) == counts["pairs"]
    ty, tx = np.unravel_index(np.argmax(tc), tc.shape)
    windows = [(int(tx) * 16 - 8, int(ty) * 16 - 8), (W // 2 - 16, H // 2 - 16), (700, 300), (1200, 650)]
    for (x0, y0) in windows:
        x0 = int(np.clip(x0, 0, W - 32)); y0 = int(np.clip(y0, 0, H - 32))
        win = (x0, y0, x0 + 32, y0 + 32)
        w4, _ = sr.render(sq, W, H, 4, window=win, s=s)
        assert np.array_equal(over[2][y0:y0 + 32, x0:x0 + 32], w4[2]), f"mode 4 window {win}"
        w0, _ = sr.render(sq, W, H, 0, window=win, s=s)
        assert_close([p[y0:y0 + 32, x0:x0 + 32] for p in planes], w0, f"C3 window {win}")


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_errors_and_empty(hiplib):
    import ctypes as C
    import torch
    from mesh2splat_amd.splat import to_c
    c = Converter(0)
    L = _lib.load()
    sk = C.c_uint64()
    for res in ((0, 10), (10, 0), (8193, 4), (4, 8193)):
        p = to_c(SplatParams(res, 0))
        assert L.m2s_splat(c._h, C.byref(p), None, 0, C.byref(sk)) == 1
    assert L.m2s_splat(c._h, C.byref(to_c(SplatParams((8, 8), 7))), None, 0, C.byref(sk)) == 1
    assert L.m2s_splat(c._h, C.byref(to_c(SplatParams((8, 8), 0))), None, 0, C.byref(sk)) == 1     # no quads
    # a previous splat leaves values behind; n = 0 clears them
    q = sr.random_quads(50, 8192, 8, 5)
    c.splat(SplatParams((8192, 8), 0), quads=torch.from_numpy(q).cuda())
    planes, n_sk = c.splat(SplatParams((8192, 8), 0), quads=torch.empty((0, 24), dtype=torch.float32, device="cuda"))
    assert n_sk == 0 and all(not p.view(np.uint8).any() for p in planes) and planes[0].shape == (8, 8192, 4)
    c.upload_quads(q)
    a, _ = c.splat(SplatParams((8192, 8), 4))
    b, _ = c.splat(SplatParams((8192, 8), 4), quads=torch.from_numpy(q).cuda())
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c.close()


# ---- CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_preview_png(tmp_path, hiplib):
    import camera
    from mesh2splat_amd import gltf_io
    from mesh2splat_amd.prepass import PrepassParams
    scene = synth.sphere_grid(2, n=5, tex_size=32)
    glb, out, png = str(tmp_path / "s.glb"), str(tmp_path / "s.ply"), str(tmp_path / "view.png")
    gltf_io.write_glb(scene, glb)
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
    r = subprocess.run([exe, glb, out, "--density", "96", "--preview", png, "--preview-size", "320x200"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = open(png, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    # chunks: IHDR, IDAT(s), IEND
    pos, idat, W, H = 8, b"", 0, 0
    while pos < len(data):
        ln = int.from_bytes(data[pos:pos + 4], "big")
        typ = data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + ln]
        assert zlib.crc32(typ + body) == int.from_bytes(data[pos + 8 + ln:pos + 12 + ln], "big")
        if typ == b"IHDR":
            W, H = int.from_bytes(body[0:4], "big"), int.from_bytes(body[4:8], "big")
            assert body[8:10] == b"\x08\x06"
        elif typ == b"IDAT":
            idat += body
        pos += 12 + ln
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 4 * W)
    assert (raw[:, 0] == 0).all()
    img = raw[:, 1:].reshape(H, W, 4)
    # the same frame through the Python path, with the camera the CLI printed (its usage() formula)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("preview camera:")][0]
    vals = dict(kv.split("=") for kv in line.split(":", 1)[1].split())
    eye = [float(v) for v in vals["eye"].split(",")]
    centre = [float(v) for v in vals["centre"].split(",")]
    near, far = float(vals["near"]), float(vals["far"])
    loaded = gltf_io.load_glb(glb)
    mn = np.min([m.bbox_min for m in loaded.meshes], 0)
    mx = np.max([m.bbox_max for m in loaded.meshes], 0)
    c_ = (mn.astype(np.float64) + mx) / 2
    radius = np.linalg.norm(mx.astype(np.float64) - mn) / 2
    dist = 1.1 * radius / np.tan(np.radians(22.5))
    assert np.allclose(centre, c_) and np.allclose(eye, c_ + [0, 0, dist]) and np.isclose(near, dist / 100) and np.isclose(far, dist * 10)
    conv = Converter(0)
    conv.upload_scene(loaded)
    conv.convert(96)
    pp = PrepassParams(view_mat=camera.look_at(eye, centre), proj_mat=camera.perspective(45.0, W / H, near, far),
                       renderer_resolution=(W, H), resolution_target=96)
    conv.prepass(pp, download=False)
    conv.sort_prepass(download=False)
    planes, _ = conv.splat(SplatParams((W, H), 0))
    conv.close()
    assert np.array_equal(img, planes[2][::-1]), "PNG != albedo plane flipped"
    assert img[..., 3].any()
