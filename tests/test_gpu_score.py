"""-m gpu: the fidelity score (m2s_relight_mesh, m2s_score_frames: k_score) through the C ABI against the numpy restatement
tests/score_ref.py — every field of the result and every byte of the error map equal, on seeded random byte images at the sizes where
the kernel's tiling (cells of 4 x 4 pixels, workgroup tiles of 64 x 64 pixels with one cell of halo, 16-byte row loads when W % 4 == 0
and the pointers are aligned) can go wrong — and Converter.relight_mesh / score / score_views on a small scene."""
import ctypes as C
import math

import numpy as np
import pytest

import camera
import score_ref as sr
from mesh2splat_amd import synth
from mesh2splat_amd.converter import Converter, _DeviceImage
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prepass import PrepassParams
from mesh2splat_amd.scene import Mesh, Scene
from mesh2splat_amd.score import ScoreParams, ScoreParamsC, ScoreResultC, orbit_cameras, pool, to_c

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 9), (8, 8), (9, 12), (37, 23), (64, 64), (200, 70), (70, 200)]     # W x H


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


_images = {}


def images(W, H, zero_cover_a=False):
    """Four seeded random (H, W, 4) byte images on the device (frames a, b; coverage planes with about half their alpha bytes zero) and
    their host copies; made once per size."""
    import torch
    key = (W, H, zero_cover_a)
    if key not in _images:
        g = torch.Generator(device="cuda")
        g.manual_seed(1000 * W + H)
        dev = [torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(4)]
        for t in dev[2:]:
            t[..., 3] *= torch.rand((H, W), device="cuda", generator=g) < 0.5
        if zero_cover_a:
            dev[2][..., 3] = 0
        torch.cuda.synchronize()
        _images[key] = (dev, [t.cpu().numpy() for t in dev])
    return _images[key]


def check(conv, W, H, mask_mode, no_cover, want_map, zero_cover_a=False, what=""):
    dev, host = images(W, H, zero_cover_a)
    flags = (sr.NO_COVER if no_cover else 0) | (sr.WANT_MAP if want_map else 0)
    want = sr.score(host[0], host[1], host[2], host[3], mask_mode, flags)
    cov = (None, None) if no_cover else (dev[2], dev[3])
    got = conv.score_frames(ScoreParams((W, H), mask_mode, no_cover, want_map), dev[0], dev[1], cov[0], cov[1], download_map=want_map)
    print(f"{what} {W}x{H} mask {mask_mode} flags {flags}: {got.integers()}")
    assert got.integers() == {k: want[k] for k in sr.FIELDS}
    if want_map:
        assert np.array_equal(got.error_map, want["map"])
    else:
        assert conv.device_score_map == 0
    p = sr.psnr(want)
    assert (math.isnan(p) and math.isnan(got.psnr)) or got.psnr == pytest.approx(p, rel=1e-12)
    return got, want


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes(conv, size):
    W, H = size
    got, want = check(conv, W, H, 2, False, True, what="size")
    if W < 8 or H < 8:
        assert got.windows == 0 and math.isnan(got.ssim)
    else:
        assert got.windows <= ((W - 8) // 4 + 1) * ((H - 8) // 4 + 1)
    assert sum(got.cover) == W * H


@pytest.mark.parametrize("size", [(37, 23), (200, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mask_mode", [0, 1, 2, 3])
@pytest.mark.parametrize("no_cover,want_map", [(False, False), (True, False), (False, True), (True, True)])
def test_mask_modes_and_flags(conv, size, mask_mode, no_cover, want_map):
    got, _ = check(conv, size[0], size[1], mask_mode, no_cover, want_map, what="modes")
    if no_cover:
        assert got.cover == (0, 0, 0, size[0] * size[1]) and got.pixels == size[0] * size[1]


def test_cover_a_all_zero(conv):
    got, _ = check(conv, 37, 23, 1, False, True, zero_cover_a=True, what="A covers nothing")
    assert got.pixels == 0 and got.windows == 0 and math.isnan(got.psnr) and math.isnan(got.ssim) and not got.error_map.any()
    assert got.cover[1] == got.cover[3] == 0 and got.coverage_iou == 0.0


def test_unaligned_pointers_take_the_narrow_loads(conv):
    """W % 4 == 0 but the images start 4 bytes off a 16-byte boundary: the kernel may not issue 16-byte loads.  Same figures."""
    import torch
    W = H = 64
    dev, host = images(W, H)
    off = []
    for t in dev:
        buf = torch.empty(W * H * 4 + 16, dtype=torch.uint8, device="cuda")
        view = buf[4:4 + W * H * 4]
        view.copy_(t.reshape(-1))
        assert view.data_ptr() % 16 == 4
        off.append(view)
    want = sr.score(host[0], host[1], host[2], host[3], 2, sr.WANT_MAP)
    got = conv.score_frames(ScoreParams((W, H), 2, False, True), *off, download_map=True)
    assert got.integers() == {k: want[k] for k in sr.FIELDS} and np.array_equal(got.error_map, want["map"])
    # ... and a _DeviceImage is accepted where a tensor is
    again = conv.score_frames(ScoreParams((W, H), 2, False, True), *[_DeviceImage(t.data_ptr(), H, W) for t in dev])
    assert again == got


def test_saturation(conv):
    """64 x 64 all 0 against all 255: the largest sums a workgroup tile can hold; nothing wraps."""
    import torch
    W = H = 64
    a = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    b = torch.full((H, W, 4), 255, dtype=torch.uint8, device="cuda")
    got = conv.score_frames(ScoreParams((W, H), 0, True, False), a, b)
    want = sr.score(a.cpu().numpy(), b.cpu().numpy(), flags=sr.NO_COVER)
    assert got.integers() == {k: want[k] for k in sr.FIELDS}
    assert got.sse == (W * H * 65025,) * 3 and got.sad == (W * H * 255,) * 3 and got.max_abs == (255,) * 3 and got.windows == 15 * 15
    assert got.psnr == pytest.approx(0.0, abs=1e-12)
    same = conv.score_frames(ScoreParams((W, H), 0, True, False), b, b)
    assert same.ssim_q32 == 225 * 2 ** 32 and same.ssim == 1.0 and same.sse == (0, 0, 0) and math.isinf(same.psnr)


def test_determinism(conv):
    dev, _ = images(200, 70)
    p = ScoreParams((200, 70), 2, False, True)
    r1 = conv.score_frames(p, *dev, download_map=True)
    r2 = conv.score_frames(p, *dev, download_map=True)
    assert r1 == r2 and np.array_equal(r1.error_map, r2.error_map)


def test_errors(hiplib):
    import torch
    L = hiplib
    img = torch.zeros((16, 16, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = img.data_ptr()
    out = ScoreResultC()
    with Converter(0) as c:
        call = lambda pc, a=ptr: L.m2s_score_frames(c._h, C.byref(pc), a, ptr, ptr, ptr, C.byref(out))
        assert call(to_c(ScoreParams((16, 16)))) == 0
        for res in ((0, 16), (8193, 16), (16, 0), (16, 8193), (-1, 16)):
            assert call(to_c(ScoreParams(res))) == 1                                   # M2S_ERR_INVALID
        assert call(to_c(ScoreParams((16, 16), mask_mode=4))) == 1
        bad = to_c(ScoreParams((16, 16)))
        bad.flags = 4
        assert call(bad) == 1
        bad = to_c(ScoreParams((16, 16)))
        bad.reserved[1] = 1
        assert call(bad) == 1
        assert L.m2s_score_frames(c._h, None, ptr, ptr, ptr, ptr, C.byref(out)) == 1
        assert L.m2s_score_frames(c._h, C.byref(to_c(ScoreParams((16, 16)))), ptr, ptr, ptr, ptr, None) == 1
        assert call(to_c(ScoreParams((16, 16))), None) == 7                            # M2S_ERR_STATE: no m2s_relight_mesh has run
        assert L.m2s_device_mesh_frame(c._h) is None
        buf = np.empty((16, 16, 4), np.uint8)
        assert L.m2s_download_mesh_frame(c._h, buf.ctypes.data, buf.nbytes) == 7
        assert call(to_c(ScoreParams((16, 16)))) == 0                                  # no WANT_MAP
        assert L.m2s_device_score_map(c._h) is None and L.m2s_download_score_map(c._h, buf.ctypes.data, buf.nbytes) == 7
        assert call(to_c(ScoreParams((16, 16), want_map=True))) == 0
        assert L.m2s_device_score_map(c._h) and L.m2s_download_score_map(c._h, buf.ctypes.data, buf.nbytes - 1) == 5     # M2S_ERR_CAPACITY
        assert L.m2s_download_score_map(c._h, buf.ctypes.data, buf.nbytes) == 0
        assert call(to_c(ScoreParams((16, 16)))) == 0 and L.m2s_device_score_map(c._h) is None      # the LAST call kept none
        lp = LightParams(renderer_resolution=(16, 16), shadow_resolution=16)
        from mesh2splat_amd import light as li
        assert L.m2s_relight_mesh(c._h, C.byref(li.to_c(lp))) == 7                     # no mesh G-buffer
        c.set_profiling(True)
        c.score_frames(ScoreParams((16, 16)), img, img, img, img)
        assert c.last_score_ms > 0
    assert C.sizeof(ScoreParamsC) == 24 and C.sizeof(ScoreResultC) == 120


# ---- the mesh frame and the score of a conversion --------------------------------------------------------------------------------
W, H, R = 48, 40, 64
NEAR_FAR = (0.05, 50.0)
EYE = (0.9, 0.8, 2.4)


def small_scene():
    """A two-triangle textured quad and, behind it to the side, one cube."""
    quad = synth.unit_quad(synth.procedural_textures(32, 5)).meshes[0]
    cube = synth.cube_sphere(1, name="cube_0").meshes[0]
    v = cube.vertices.copy()
    v[:, 0:3] = v[:, 0:3] * np.float32(0.35) + np.float32([1.3, 0.5, -0.6])
    return Scene([Mesh(quad.name, quad.vertices, quad.base_color, quad.textures), Mesh("cube_0", v, (0.9, 0.4, 0.2, 1.0))])


@pytest.fixture(scope="module")
def frame(conv):
    conv.upload_scene(small_scene())
    conv.convert(R)
    pp = PrepassParams(view_mat=camera.look_at(EYE, (0.7, 0.5, 0.0)), proj_mat=camera.perspective(50.0, W / H, *NEAR_FAR), renderer_resolution=(W, H),
                       near_plane=NEAR_FAR[0], far_plane=NEAR_FAR[1], resolution_target=R, render_mode=0)
    lp = LightParams(light_position=(1.5, 2.0, 3.0), camera_position=EYE, near_plane=NEAR_FAR[0], far_plane=NEAR_FAR[1], renderer_resolution=(W, H),
                     shadow_resolution=128, want_shadow_counts=True)
    return pp, lp


def test_relight_mesh(conv, frame):
    from mesh2splat_amd import light as li
    pp, lp = frame
    splat_frame, splat_counts = conv.render_frame(pp, lp)
    conv.mesh_render(pp, download=False)
    mesh_frame = conv.relight_mesh(lp)
    assert conv.device_mesh_frame and conv.device_mesh_frame != conv.device_frame
    # device_frame's bytes and the shadow counts of the last relight are unchanged by the call
    kept, counts = conv._download_relit(li.to_c(lp))
    assert np.array_equal(kept, splat_frame) and np.array_equal(counts, splat_counts)
    # ... it equals relight_split(1.0) in columns [0, W - 1)
    split, _ = conv.relight_split(lp, 1.0)
    assert np.array_equal(mesh_frame[:, :W - 1], split[:, :W - 1]) and (split[:, W - 1] == 255).all()
    # ... and, byte for byte, upload_gbuffer(the mesh G-buffer) + relight
    planes = conv.download_mesh_gbuffer()
    assert (planes[2][..., 3] == 255).any() and (planes[2][..., 3] == 0).any()
    conv.upload_gbuffer(planes)
    by_definition, _ = conv.relight(lp)
    assert np.array_equal(mesh_frame, by_definition)
    assert (mesh_frame != splat_frame).any()


def test_converter_score(conv, frame):
    from mesh2splat_amd import light as li
    pp, lp = frame
    for mask_mode in (2, 3):
        got = conv.score(pp, lp, mask_mode=mask_mode, want_map=True)
        splat_frame, _ = conv._download_relit(li.to_c(lp))
        mesh_frame = conv.download_mesh_frame(W, H)
        cover_a, cover_b = conv.download_mesh_gbuffer()[2], conv.download_gbuffer()[2]
        want = sr.score(mesh_frame, splat_frame, cover_a, cover_b, mask_mode, sr.WANT_MAP)
        print(f"mask {mask_mode}: {got.integers()}, psnr {got.psnr:.2f} dB, ssim {got.ssim:.4f}, coverage IoU {got.coverage_iou:.4f}")
        assert got.integers() == {k: want[k] for k in sr.FIELDS} and np.array_equal(got.error_map, want["map"])
        assert got.cover[3] > 0 and got.cover[1] + got.cover[3] > W * H // 20 and got.windows > 0 and 0.0 < got.coverage_iou <= 1.0
    # the same splats against themselves: nothing differs
    conv.render_frame(pp, lp, download=False)
    same = conv.score_frames(ScoreParams((W, H), 0, True), _DeviceImage(conv.device_frame, H, W), None)
    assert same.sse == (0, 0, 0) and same.ssim == 1.0


def test_score_views(conv, frame):
    scene = small_scene()
    cams = orbit_cameras(scene, 3, W, H, elevation_deg=20.0)
    light = (2.0, 2.5, 3.0)
    views, pooled = conv.score_views(cams, R, light, 30.0, shadow_resolution=128)
    assert len(views) == 3 and pooled == pool(views)
    for name, n in (("cover", 4), ("sse", 3), ("sad", 3)):
        assert getattr(pooled, name) == tuple(sum(getattr(v, name)[i] for v in views) for i in range(n))
    assert pooled.pixels == sum(v.pixels for v in views) and pooled.windows == sum(v.windows for v in views)
    assert pooled.ssim_q32 == sum(v.ssim_q32 for v in views) and pooled.max_abs == tuple(max(v.max_abs[i] for v in views) for i in range(3))
    assert pooled.ssim == pooled.ssim_q32 / 2 ** 32 / pooled.windows and len({v.integers()["pixels"] for v in views}) > 1
    # one of the views again, by hand
    pp, lp = cams[1].frame_params(R, light, 30.0, shadow_resolution=128)
    assert conv.score(pp, lp) == views[1]
