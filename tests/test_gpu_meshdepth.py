"""-m gpu: the mesh depth prepass (m2s_mesh_depth, k_md_*) through the C ABI against the numpy restatement tests/meshdepth_ref.py
(which tests/test_meshdepth_cpu.py holds to a float64 ray cast): images bit-identical, counts equal, both raster paths the same bytes,
and the image as the occluder of the viewer prepass, end to end."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import camera
import meshdepth_ref as mr
import test_meshdepth_cpu as cpu
from mesh2splat_amd import _lib, synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.meshdepth import MeshDepthParams, MeshDepthParamsC, to_c
from mesh2splat_amd.prepass import PrepassParams
from mesh2splat_amd.scene import Mesh, Scene

pytestmark = pytest.mark.gpu
F = np.float32
EYE = np.eye(4, dtype=F)
# scale (2, 0.5, 4), a quarter turn about z, a translation: the matrix tests/test_gpu_light.py calls EXACT_MODEL
EXACT_MODEL = np.array([[0, 2, 0, 0], [-0.5, 0, 0, 0], [0, 0, 4, 0], [0.5, -0.25, 0.125, 1]], F)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def mesh_of(tris, alpha=1.0, name="m"):
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    v = np.zeros((len(tris) * 3, 12), F)
    v[:, 0:3] = tris.reshape(-1, 3)
    v[:, 5] = 1
    v[:, 6] = 1
    v[:, 9] = 1
    return Mesh(name, v, base_color=(0.7, 0.6, 0.5, alpha))


def check(conv, scene, proj, view, model, W, H, what=""):
    """Upload, run, compare image and counts with the restatement -> (image, counts, restatement)."""
    conv.upload_scene(scene)
    img, counts = conv.mesh_depth(MeshDepthParams(view, proj, model, (W, H)))
    pos, opaque = mr.scene_triangles(scene)
    r = mr.mesh_depth(pos, opaque, proj, view, model, W, H, want_winner=False)
    diff = int((img.view(np.uint32) != r["image"].view(np.uint32)).sum())
    got = [counts[k] for k in ("drawn", "clipped", "non_finite", "pairs")]
    print(f"{what}: {W}x{H}, {len(pos)} triangles, texels that differ {diff}, counts {got} / restatement {r['counts']}, "
          f"texel updates {counts['texel_updates']}")
    assert same_bits(img, r["image"]), f"{what}: {diff} texels differ"
    assert got == r["counts"], what
    assert img.min() >= 0 and img.max() <= 1
    return img, counts, r


# ---- 5. bit-identical to the restatement -----------------------------------------------------------------------------------------------
def test_scene_of_the_ray_cast_test(conv):
    W, H = 384, 216
    proj, view = cpu.view_camera((W, H))
    img, counts, r = check(conv, Scene([mesh_of(cpu.wall_floor_ico())]), proj, view, EYE, W, H, "wall + floor + icosahedron")
    assert counts["clipped"] == 2 and counts["drawn"] >= 5 and (img < 1).mean() > 0.5


@pytest.mark.parametrize("shape", ["fan", "strip"])
def test_shared_edges(conv, shape):
    W = H = 64
    pos = cpu.screen_tris(cpu.fan_px() if shape == "fan" else cpu.strip_px(), W, H)
    img, _, r = check(conv, Scene([mesh_of(pos)]), EYE, EYE, EYE, W, H, shape)
    flipped, _, _ = check(conv, Scene([mesh_of(pos[:, ::-1])]), EYE, EYE, EYE, W, H, shape + " flipped")
    assert same_bits(img, flipped)
    assert ((img < 1) == (r["frags"] == 1)).all()


def test_clipped_triangles(conv):
    W, H = 384, 216
    proj, view = cpu.view_camera((W, H))
    one = [(-1.0, 0.2, -1.0), (1.5, 0.4, -1.5), (0.2, 0.9, 6.0)]
    two = [(0.1, 0.5, -3.0), (-2.0, 0.2, 7.0), (2.5, 1.6, 5.0)]
    guard = [(-3000.0, -20.0, -5.0), (3000.0, -20.0, -5.0), (0.0, 40.0, -5.0)]
    behind = [(-1.0, 0.0, 6.0), (1.0, 0.0, 6.0), (0.0, 1.0, 7.0)]
    for name, tris in (("one behind", [one]), ("two behind", [two]), ("guard band", [guard]), ("all", [one, two, guard, behind])):
        check(conv, Scene([mesh_of(tris)]), proj, view, EYE, W, H, name)
    proj20, _ = cpu.view_camera((W, H), far=20.0)
    img, counts, _ = check(conv, Scene([mesh_of([[(-5, -5, -30.0), (5, -5, -30.0), (0, 5, -40.0)]])]), proj20, view, EYE, W, H, "beyond far")
    assert (img == 1).all() and counts["drawn"] == 0 and counts["texel_updates"] == 0
    for bad in (np.nan, np.inf):
        img, counts, _ = check(conv, Scene([mesh_of([[(-1, 0, 0.0), (bad, 0, 0.0), (0, 2, 0.0)], [(-1, 0, 0.0), (1, 0, 0.0), (0, 2, 0.0)]])]),
                               proj, view, EYE, W, H, f"vertex {bad}")
        assert counts["non_finite"] == 1 and counts["drawn"] == 1


def test_mesh_selection(conv):
    W, H = 96, 64
    proj, view = cpu.view_camera((W, H))
    a = [[(-1, 0.2, 0.0), (1, 0.2, 0.0), (0, 2, 0.0)]]
    b = [[(-2, 0.1, 1.0), (0, 0.1, 1.0), (-1, 1.5, 1.0)]]
    both, _, _ = check(conv, Scene([mesh_of(a, 1.0), mesh_of(b, 0.999)]), proj, view, EYE, W, H, "alpha 1 + alpha 0.999")
    only, _, _ = check(conv, Scene([mesh_of(a, 1.0)]), proj, view, EYE, W, H, "alpha 1")
    assert same_bits(both, only)
    none, counts, _ = check(conv, Scene([mesh_of(a, 0.999), mesh_of(b, 0.5)]), proj, view, EYE, W, H, "no opaque mesh")
    assert (none == 1).all() and counts["drawn"] == 0


def soup(n, seed):
    """Triangles of mixed sizes: sub-pixel to window-filling, some crossing the near plane, some behind the camera."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, (n, 1, 3)) * (1, 0.6, 2.5)
    size = 10.0 ** rng.uniform(-3, 0.7, (n, 1, 1))
    return (c + rng.uniform(-1, 1, (n, 3, 3)) * size).astype(F)


@pytest.mark.parametrize("res", [(384, 216), (97, 61), (333, 219)])
def test_random_soup_with_a_model_matrix(conv, res):
    W, H = res
    proj, view = cpu.view_camera((W, H), eye=(0.4, 0.7, 3.0))
    model = (EXACT_MODEL.astype(np.float64) * 0.5).astype(F)
    model[3, 3] = 1
    img, counts, _ = check(conv, Scene([mesh_of(soup(2000, 7))]), proj, view, model, W, H, "soup")
    # (check() has held every count to the restatement's; these only show that the soup reaches the clipper, the binned path and the
    #  in-place path at every window size — how many triangles cover a pixel centre depends on the resolution)
    assert counts["clipped"] > 10 and counts["pairs"] > 0 and counts["drawn"] > counts["clipped"]


@pytest.mark.parametrize("res", [(97, 61), (1920, 1080)])
def test_synth_sphere(conv, res):
    W, H = res
    proj = camera.perspective(60.0, W / H, 0.1, 50.0)
    view = camera.look_at((0.3, 0.4, 2.6), (0, 0, 0))
    img, counts, _ = check(conv, synth.cube_sphere(12), proj, view, EYE, W, H, "cube sphere")
    assert counts["drawn"] > 100 and 0.1 < (img < 1).mean() < 0.9       # (the sphere's disc fills about a fifth of the window)


# ---- 6. both paths give the same bytes ---------------------------------------------------------------------------------------------------
def both_paths(conv, scene, proj, view, model, W, H, what):
    conv.upload_scene(scene)
    p = MeshDepthParams(view, proj, model, (W, H))
    out = {}
    try:
        for box in (0, 8192, -1):
            conv.debug_set_mesh_depth_inplace(box)
            out[box] = conv.mesh_depth(p)
    finally:
        conv.debug_set_mesh_depth_inplace(-1)
    print(what, {b: (c["pairs"], c["texel_updates"]) for b, (_, c) in out.items()})
    assert same_bits(out[0][0], out[8192][0]) and same_bits(out[0][0], out[-1][0]), what
    assert out[0][1]["drawn"] == out[8192][1]["drawn"] == out[-1][1]["drawn"]
    return out


def test_both_paths_scene_of_the_ray_cast_test(conv):
    W, H = 384, 216
    proj, view = cpu.view_camera((W, H))
    out = both_paths(conv, Scene([mesh_of(cpu.wall_floor_ico())]), proj, view, EYE, W, H, "wall + floor + icosahedron")
    assert out[0][1]["pairs"] > out[8192][1]["pairs"] > 0          # (the clipped floor is binned whatever the threshold)


def test_both_paths_one_window_filling_triangle(conv):
    W, H = 640, 360
    out = both_paths(conv, Scene([mesh_of([[(-1.9, -1.9, 0.25), (1.9, -1.9, 0.5), (0.0, 1.95, -0.5)]])]), EYE, EYE, EYE, W, H, "one triangle")
    assert out[8192][1]["pairs"] == 0 and out[0][1]["pairs"] == ((W + 15) // 16) * ((H + 15) // 16)
    assert (out[0][0] < 1).mean() > 0.45


def test_both_paths_many_sub_pixel_triangles(conv):
    W, H = 640, 360
    rng = np.random.default_rng(3)
    n = 200_000
    c = rng.uniform(-0.98, 0.98, (n, 1, 3))
    pos = (c + rng.uniform(-1, 1, (n, 3, 3)) * (1.2 / W, 1.2 / H, 0.01)).astype(F)
    out = both_paths(conv, Scene([mesh_of(pos)]), EYE, EYE, EYE, W, H, "200 000 sub-pixel triangles")
    assert out[-1][1]["pairs"] == 0 and 1000 < out[-1][1]["drawn"] < n
    r = mr.mesh_depth(pos, np.ones(n, bool), EYE, EYE, EYE, W, H, want_winner=False)
    assert same_bits(out[-1][0], r["image"]) and out[-1][1]["drawn"] == r["counts"][0]


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------------
def occluder_scene():
    """An opaque wall at z = 0; a sphere behind it and one in front, both with alpha 0.999: depth-tested Gaussians (alpha > .95) that are
    no occluders themselves."""
    wall = Mesh("wall", synth.patch_vertices(4, 4, (-2, -2, 0), (4, 0, 0), (0, 4, 0)), base_color=(0.5, 0.5, 0.5, 1.0))
    hidden = Mesh("hidden", synth.cube_sphere_vertices(6, 0.4, (0.3, 0.1, -1.0)), base_color=(0.9, 0.2, 0.2, 0.999))
    front = Mesh("front", synth.cube_sphere_vertices(6, 0.3, (-0.4, 0.2, 1.0)), base_color=(0.2, 0.9, 0.2, 0.999))
    return Scene([wall, hidden, front])


def frame_params(res):
    W, H = res
    proj = camera.perspective(60.0, W / H, 0.1, 50.0)
    view = camera.look_at((0.1, 0.2, 3.5), (0, 0, 0))
    return PrepassParams(view_mat=view, proj_mat=proj, renderer_resolution=res, near_plane=0.1, far_plane=50.0, resolution_target=64)


def test_mesh_as_occluder_end_to_end(conv, oracle):
    res = (320, 200)
    scene = occluder_scene()
    conv.upload_scene(scene)
    n = conv.convert(64)
    rec = conv.download()
    assert n == len(rec) > 1000
    p = frame_params(res)
    img, counts = conv.mesh_depth(p)
    pos, opaque = mr.scene_triangles(scene)
    r = mr.mesh_depth(pos, opaque, p.proj_mat, p.view_mat, p.model_mat, res[0], res[1], want_winner=False)
    assert same_bits(img, r["image"]) and counts["drawn"] == 32
    want = oracle.prepass(replace(p, perform_mesh_depth_test=True, mesh_depth=r["image"]), rec)
    pd = conv._with_device_mesh_depth(p)
    vis, quads, depths = conv.prepass(pd)
    assert vis == want[0] and same_bits(quads, want[1]) and same_bits(depths, want[2])
    z = quads[:, 20 + 2]                                  # ws_pos.z of the survivors
    is_hidden, is_front = rec[:, 2] < -0.5, rec[:, 2] > 0.5
    assert is_hidden.sum() > 100 and is_front.sum() > 100
    assert (z < -0.5).sum() == 0                          # every Gaussian of the hidden object is culled
    assert (z > 0.5).sum() == is_front.sum()              # every Gaussian of the front object is kept
    without = conv.prepass(p)[0]
    assert without >= vis + is_hidden.sum()
    # the same through the fused prepass + sort
    sq = conv.prepass_sorted(pd)
    assert sq.shape[0] == vis and (sq[:, 22] < -0.5).sum() == 0 and (sq[:, 22] > 0.5).sum() == is_front.sum()
    order = np.argsort(depths.view(np.uint32), kind="stable")
    assert same_bits(sq, quads[order])


def test_render_frame_with_and_without_the_occluder(conv):
    res = (320, 200)
    conv.upload_scene(occluder_scene())
    conv.convert(64)
    p = frame_params(res)
    lp = LightParams(light_position=(0.5, 1.5, 3.0), camera_position=(0.1, 0.2, 3.5), near_plane=0.1, far_plane=50.0, renderer_resolution=res,
                     shadow_resolution=128)
    off = conv.render_frame(p, lp)
    assert (conv.render_frame(p, lp, mesh_depth_test=False) == off).all()
    # today's frame, by hand: the flag off must not change a byte
    from mesh2splat_amd.splat import SplatParams
    conv.prepass(p, download=False)
    conv.sort_prepass(download=False)
    conv.splat(SplatParams(res, 0), download=False)
    conv.shadow(p, lp, download=False)
    assert (conv.relight(lp) == off).all()
    on = conv.render_frame(p, lp, mesh_depth_test=True)
    assert on.shape == off.shape
    # and it is the frame of the culled quads
    conv.mesh_depth(p, download=False)
    conv.prepass_sorted(conv._with_device_mesh_depth(p), download=False)
    conv.splat(SplatParams(res, 0), download=False)
    conv.shadow(p, lp, download=False)
    assert (conv.relight(lp) == on).all()


# ---- 8. triangle range -------------------------------------------------------------------------------------------------------------------
def test_triangle_range_halves_combine_by_min(hiplib):
    W, H = 384, 216
    proj, view = cpu.view_camera((W, H))
    scene = Scene([mesh_of(cpu.wall_floor_ico()[:7], name="a"), mesh_of(soup(500, 2), name="b")])
    p = MeshDepthParams(view, proj, EYE, (W, H))
    n = scene.n_triangles
    with Converter(0) as c:
        c.upload_scene(scene)
        whole, cw = c.mesh_depth(p)
        parts, drawn = [], 0
        for first, count in ((0, 100), (100, n - 100)):
            c.set_triangle_range(first, count)
            c.upload_scene(scene)
            img, cnt = c.mesh_depth(p)
            parts.append(img)
            drawn += cnt["drawn"]
    assert same_bits(np.minimum(parts[0], parts[1]), whole) and drawn == cw["drawn"]
    assert not same_bits(parts[0], whole) and not same_bits(parts[1], whole)


# ---- 9. errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors(hiplib):
    L = hiplib
    with Converter(0) as c:
        ok = to_c(MeshDepthParams(EYE, EYE, EYE, (64, 64)))
        assert L.m2s_device_mesh_depth(c._h) is None
        assert L.m2s_mesh_depth(c._h, C.byref(ok), None) == 7                       # M2S_ERR_STATE: no scene
        buf = np.empty(64 * 64, F)
        assert L.m2s_download_mesh_depth(c._h, buf.ctypes.data, buf.size) == 7      # no image yet
        c.upload_scene(Scene([mesh_of([[(-1, -1, 0), (1, -1, 0), (0, 1, 0)]])]))
        for res in ((0, 64), (64, 0), (8193, 64), (64, 8193), (-1, 64)):
            assert L.m2s_mesh_depth(c._h, C.byref(to_c(MeshDepthParams(EYE, EYE, EYE, res))), None) == 1   # M2S_ERR_INVALID
        for k in (0, 1):
            bad = to_c(MeshDepthParams(EYE, EYE, EYE, (64, 64)))
            bad.reserved[k] = 1
            assert L.m2s_mesh_depth(c._h, C.byref(bad), None) == 1
        assert L.m2s_mesh_depth(None, C.byref(ok), None) == 1 and L.m2s_mesh_depth(c._h, None, None) == 1
        assert L.m2s_debug_set_mesh_depth_inplace(c._h, 8193) == 1 and L.m2s_debug_set_mesh_depth_inplace(c._h, -2) == 1
        assert L.m2s_mesh_depth(c._h, C.byref(ok), None) == 0                       # out_counts may be NULL
        assert L.m2s_device_mesh_depth(c._h)
        assert L.m2s_download_mesh_depth(c._h, buf.ctypes.data, buf.size - 1) == 5  # M2S_ERR_CAPACITY
        assert L.m2s_download_mesh_depth(c._h, buf.ctypes.data, buf.size) == 0 and (buf < 1).any()
        v = (C.c_uint64 * 5)()
        assert L.m2s_last_mesh_depth_counts(c._h, v) == 0 and v[0] == 1
        c.set_profiling(True)
        c.mesh_depth(MeshDepthParams(EYE, EYE, EYE, (8192, 8192)), download=False)  # the largest window: 262 144 pairs from one triangle
        assert c.last_mesh_depth_ms > 0 and set(c.last_mesh_depth_stage_ms()) == {"setup", "bin", "raster"}
    assert C.sizeof(MeshDepthParamsC) == 3 * 64 + 16
    for name in ("m2s_mesh_depth", "m2s_device_mesh_depth", "m2s_download_mesh_depth", "m2s_last_mesh_depth_ms", "m2s_last_mesh_depth_stage_ms",
                 "m2s_last_mesh_depth_counts"):
        assert name in _lib.EXPORTS and hasattr(L, name)


def test_cli_mesh_depth_test_flag(hiplib, tmp_path):
    import hashlib
    import os
    import re
    import subprocess
    from mesh2splat_amd import gltf_io
    scene = synth.sphere_grid(2, n=5, tex_size=32)
    glb, out = str(tmp_path / "s.glb"), str(tmp_path / "s.ply")
    plain, occl, plain2 = (str(tmp_path / n) for n in ("view.png", "occluded.png", "view2.png"))
    gltf_io.write_glb(scene, glb)
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
    base = [exe, glb, out, "--density", "96", "--preview-size", "320x200"]
    r0 = subprocess.run(base + ["--preview", plain], capture_output=True, text=True, timeout=300)
    r1 = subprocess.run(base + ["--preview", occl, "--mesh-depth-test"], capture_output=True, text=True, timeout=300)
    r2 = subprocess.run(base + ["--preview", plain2], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r1.returncode == 0 and r2.returncode == 0, r1.stderr
    assert "mesh depth test:" not in r0.stdout
    m = re.search(r"mesh depth test: (\d+) triangles drawn \((\d+) clipped\), (\d+) Gaussians pass", r1.stdout)
    n0 = int(re.search(r"preview 320x200: (\d+) quads splatted", r0.stdout).group(1))
    assert m and int(m.group(1)) > 100 and 0 < int(m.group(3)) < n0          # spheres hide their own far side and each other
    assert f"preview 320x200: {m.group(3)} quads splatted" in r1.stdout
    assert open(occl, "rb").read()[:8] == b"\x89PNG\r\n\x1a\n"
    assert hashlib.sha256(open(plain, "rb").read()).digest() == hashlib.sha256(open(plain2, "rb").read()).digest()
