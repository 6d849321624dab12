"""-m gpu: the mesh render pass (m2s_mesh_render: k_md_* with the 64-bit payload, k_mr_shade) and the split-screen relighting
(m2s_relight_split) through the C ABI against the numpy restatement tests/meshrender_ref.py, which tests/test_meshrender_cpu.py holds
to a float64 ray cast: visibility images equal as uint64, counts equal, both raster paths the same bytes, the five planes within one
output step of the float64 evaluation on well-conditioned pixels, the split frame byte-identical to m2s_relight of either G-buffer.

Measured: see DESIGN 5.11 (the planes' maximum and the excluded share are printed by test_planes)."""
import ctypes as C

import numpy as np
import pytest

import camera
import meshrender_ref as rr
import test_meshdepth_cpu as cpu
import test_meshrender_cpu as mcpu
from mesh2splat_amd import _lib, synth
from mesh2splat_amd.converter import Converter, GaussianRelightingPass, MeshRenderPass, RenderContext
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.meshrender import EMPTY, MeshRenderParams, MeshRenderParamsC, to_c
from mesh2splat_amd.prepass import PrepassParams
from mesh2splat_amd.scene import Scene

pytestmark = pytest.mark.gpu
F = np.float32
EYE = np.eye(4, dtype=F)
EXACT_MODEL = np.array([[0, 2, 0, 0], [-0.5, 0, 0, 0], [0, 0, 4, 0], [0.5, -0.25, 0.125, 1]], F)
NEAR_FAR = mcpu.NEAR_FAR
mesh_of = mcpu.mesh_of


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def params(proj, view, model, W, H, mode=0):
    return MeshRenderParams(view, proj, model, (W, H), NEAR_FAR, mode)


def check_vis(conv, scene, proj, view, model, W, H, what=""):
    """Upload, run, compare the visibility image and the counts with the restatement -> (vis, counts, restatement)."""
    conv.upload_scene(scene)
    counts = conv.mesh_render(params(proj, view, model, W, H), download=False)
    vis = conv.download_mesh_visibility()
    pos = rr.scene_arrays(scene)["pos"]
    r = rr.visibility(pos, proj, view, model, W, H)
    got = [counts[k] for k in rr.COUNT_NAMES]
    diff = int((vis != r["vis"]).sum())
    print(f"{what}: {W}x{H}, {len(pos)} triangles, pixels that differ {diff}, counts {got} / restatement {r['counts']}")
    assert vis.dtype == np.uint64 and diff == 0, f"{what}: {diff} pixels differ"
    assert got == r["counts"], what
    return vis, counts, r


# ---- 1. the visibility image ----------------------------------------------------------------------------------------------------------------
def test_visibility_scene_of_the_ray_cast_test(conv):
    W, H = 384, 216
    proj, view = cpu.view_camera((W, H))
    vis, counts, r = check_vis(conv, Scene([mesh_of(cpu.wall_floor_ico())]), proj, view, EYE, W, H, "wall + floor + icosahedron")
    assert counts["clipped"] == 2 and counts["culled"] >= 8 and (vis != EMPTY).mean() > 0.5


@pytest.mark.parametrize("shape", ["fan", "strip"])
def test_visibility_shared_edges(conv, shape):
    W = H = 64
    pos = cpu.screen_tris(cpu.fan_px() if shape == "fan" else cpu.strip_px(), W, H)
    vis, counts, r = check_vis(conv, Scene([mesh_of(pos)]), EYE, EYE, EYE, W, H, shape)
    assert ((vis != EMPTY) == (r["frags"] == 1)).all()
    back, counts, _ = check_vis(conv, Scene([mesh_of(pos[:, ::-1])]), EYE, EYE, EYE, W, H, shape + " reversed")
    assert (back == EMPTY).all() and counts["drawn"] == 0 and counts["culled"] > 0


def test_visibility_clipped_triangles(conv):
    W, H = 384, 216
    proj, view = cpu.view_camera((W, H))
    one = [(-1.0, 0.2, -1.0), (1.5, 0.4, -1.5), (0.2, 0.9, 6.0)]
    two = [(0.1, 0.5, -3.0), (-2.0, 0.2, 7.0), (2.5, 1.6, 5.0)]
    for name, tris in (("one behind", [one]), ("two behind", [two]), ("one behind, reversed", [one[::-1]]), ("both", [one, two, two[::-1]])):
        vis, counts, _ = check_vis(conv, Scene([mesh_of(tris)]), proj, view, EYE, W, H, name)
        assert counts["clipped"] == len(tris)
    assert counts["drawn"] + counts["culled"] == 3


@pytest.mark.parametrize("res", [(97, 61), (333, 219)])
def test_visibility_random_soup_with_a_model_matrix(conv, res):
    W, H = res
    rng = np.random.default_rng(7)
    n = 2000
    c = rng.uniform(-3, 3, (n, 1, 3)) * (1, 0.6, 2.5)
    soup = (c + rng.uniform(-1, 1, (n, 3, 3)) * 10.0 ** rng.uniform(-3, 0.7, (n, 1, 1))).astype(F)
    proj, view = cpu.view_camera((W, H), eye=(0.4, 0.7, 3.0))
    model = (EXACT_MODEL.astype(np.float64) * 0.5).astype(F)
    model[3, 3] = 1
    _, counts, _ = check_vis(conv, Scene([mesh_of(soup[:1200], name="a"), mesh_of(soup[1200:], alpha=0.3, name="b")]), proj, view, model, W, H, "soup")
    assert counts["clipped"] > 10 and counts["pairs"] > 0 and counts["culled"] > 100 and counts["drawn"] > counts["clipped"]


def both_paths(conv, scene, proj, view, model, W, H, what):
    conv.upload_scene(scene)
    out = {}
    try:
        for box in (0, 8192, -1):
            conv.debug_set_mesh_depth_inplace(box)
            counts = conv.mesh_render(params(proj, view, model, W, H), download=False)
            out[box] = (conv.download_mesh_visibility(), counts)
    finally:
        conv.debug_set_mesh_depth_inplace(-1)
    print(what, {b: (c["pairs"], c["texel_updates"]) for b, (_, c) in out.items()})
    assert (out[0][0] == out[8192][0]).all() and (out[0][0] == out[-1][0]).all(), what
    assert out[0][1]["drawn"] == out[8192][1]["drawn"] == out[-1][1]["drawn"] and out[0][1]["culled"] == out[-1][1]["culled"]
    return out


def test_both_paths_one_window_filling_triangle(conv):
    W, H = 640, 360
    out = both_paths(conv, Scene([mesh_of([[(-1.9, -1.9, 0.25), (1.9, -1.9, 0.5), (0.0, 1.95, -0.5)]])]), EYE, EYE, EYE, W, H, "one triangle")
    assert out[8192][1]["pairs"] == 0 and out[0][1]["pairs"] == ((W + 15) // 16) * ((H + 15) // 16)
    assert (out[0][0] != EMPTY).mean() > 0.45


def test_both_paths_many_sub_pixel_triangles(conv):
    W, H = 640, 360
    rng = np.random.default_rng(3)
    n = 200_000
    c = rng.uniform(-0.98, 0.98, (n, 1, 3))
    pos = (c + rng.uniform(-1, 1, (n, 3, 3)) * (1.2 / W, 1.2 / H, 0.01)).astype(F)
    out = both_paths(conv, Scene([mesh_of(pos)]), EYE, EYE, EYE, W, H, "200 000 sub-pixel triangles")
    assert out[-1][1]["pairs"] == 0 and 500 < out[-1][1]["drawn"] < n
    r = rr.visibility(pos, EYE, EYE, EYE, W, H)
    assert (out[-1][0] == r["vis"]).all() and out[-1][1]["drawn"] == r["counts"][0] and out[-1][1]["culled"] == r["counts"][4]


def test_triangle_range_halves_combine_by_min(hiplib):
    W, H = 384, 216
    proj, view = cpu.view_camera((W, H))
    rng = np.random.default_rng(2)
    soup = (rng.uniform(-2, 2, (500, 1, 3)) + rng.uniform(-1, 1, (500, 3, 3)) * 0.3).astype(F)
    scene = Scene([mesh_of(cpu.wall_floor_ico()[:7], name="a"), mesh_of(soup, name="b")])
    p = params(proj, view, EYE, W, H)
    n = scene.n_triangles
    with Converter(0) as c:
        c.upload_scene(scene)
        cw = c.mesh_render(p, download=False)
        whole = c.download_mesh_visibility()
        parts, drawn = [], 0
        for first, count in ((0, 100), (100, n - 100)):
            c.set_triangle_range(first, count)
            c.upload_scene(scene)
            drawn += c.mesh_render(p, download=False)["drawn"]
            parts.append(c.download_mesh_visibility())
    assert (np.minimum(parts[0], parts[1]) == whole).all() and drawn == cw["drawn"]
    assert (parts[0] != whole).any() and (parts[1] != whole).any()
    assert ((parts[1] & np.uint64(0xFFFFFFFF))[parts[1] != EMPTY] >= 100).all()          # the index in the key is global


# ---- 2. the five planes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mcpu.gpu_plane_cases()))
def test_planes(conv, name):
    """On well-conditioned pixels every plane is within one output step of the float64 evaluation: one half-precision step for planes
    0, 1 and 3, 1 LSB for planes 2 and 4 (fp32 error is orders below a half step: a correct kernel differs only where rounding
    straddles)."""
    scene, proj, view, model, W, H, mode = mcpu.gpu_plane_cases()[name]
    ref = mcpu.reference(name)
    conv.upload_scene(scene)
    planes, counts = conv.mesh_render(params(proj, view, model, W, H, mode))
    vis = conv.download_mesh_visibility()
    assert (vis == ref["vis"]["vis"]).all(), name
    steps = rr.plane_steps(planes, ref["exact"]["planes"])
    well = ref["well"]
    pinned = rr.plane_steps(planes, ref["pinned"]["planes"])
    print(f"{name}: covered {(vis != EMPTY).sum()} px; max steps from the float64 evaluation on well-conditioned pixels {steps[well].max()}, "
          f"pixels one step off {(steps[well] == 1).sum()}, excluded share {100 * (~well).mean():.3f} %; from the fp32 restatement: max {pinned.max()}")
    assert steps[well].max() <= 1
    empty = vis == EMPTY
    for k in range(5):
        assert planes[k].shape == (H, W, 4) and (planes[k][empty].view(np.uint8) == 0).all()
    assert (planes[2][~empty][:, 3] == 255).all() and (planes[4][~empty][:, 2:] == (0, 255)).all()
    assert (planes[0][~empty][:, 3] == 1).all() and (planes[1][~empty][:, 3] == 1).all() and (planes[3][~empty][:, 3] == 1).all()


def test_empty_scene(hiplib):
    """A scene without a triangle (the empty shard of m2s_set_triangle_range): the pass is its clear."""
    W, H = 97, 61
    proj, view = cpu.view_camera((W, H))
    with Converter(0) as c:
        c.set_triangle_range(0, 0)
        c.upload_scene(Scene([mesh_of(cpu.wall_floor_ico())]))
        assert c.num_triangles == 0
        planes, counts = c.mesh_render(params(proj, view, EYE, W, H))
        assert all((p.view(np.uint8) == 0).all() for p in planes) and (c.download_mesh_visibility() == EMPTY).all()
        assert all(v == 0 for v in counts.values())


def test_nothing_drawn_and_empty_pixels(conv):
    """A scene none of whose triangles reaches a pixel (one behind the camera, one back-facing, one beyond the far plane): the pass is
    its clear — zeros in all five planes."""
    W, H = 97, 61
    proj, view = cpu.view_camera((W, H), far=20.0)
    tris = [[(-1.0, 0.0, 6.0), (1.0, 0.0, 6.0), (0.0, 1.0, 7.0)], [(0, 2, 0.0), (1, 0.2, 0.0), (-1, 0.2, 0.0)], [(-5, -5, -30.0), (5, -5, -30.0), (0, 5, -40.0)]]
    conv.upload_scene(Scene([mesh_of(tris)]))
    planes, counts = conv.mesh_render(params(proj, view, EYE, W, H))
    assert all((p.view(np.uint8) == 0).all() for p in planes) and (conv.download_mesh_visibility() == EMPTY).all()
    assert counts["drawn"] == 0 and counts["culled"] == 1 and counts["texel_updates"] == 0


def test_reference_shaped_pass(conv):
    scene, proj, view, model, W, H, mode = mcpu.gpu_plane_cases()["three materials, mode 0"]
    ctx = RenderContext(scene)
    ctx.converter = conv
    conv.upload_scene(scene)
    ctx._uploaded_scene = scene
    ctx.prepassParams = PrepassParams(view_mat=view, proj_mat=proj, model_mat=model, renderer_resolution=(W, H), near_plane=NEAR_FAR[0],
                                      far_plane=NEAR_FAR[1], resolution_target=32)
    MeshRenderPass().execute(ctx)
    want, _ = conv.mesh_render(params(proj, view, model, W, H, 0))
    assert all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(ctx.meshGBuffer, want))


# ---- 3. split screen ----------------------------------------------------------------------------------------------------------------------
def split_setup(conv):
    W, H = 97, 61
    scene = mcpu.three_materials()
    conv.upload_scene(scene)
    conv.convert(48)
    view = camera.look_at((0.2, 0.5, 3.0), (0, 0, 0))
    p = PrepassParams(view_mat=view, proj_mat=camera.perspective(50.0, W / H, *NEAR_FAR), renderer_resolution=(W, H), near_plane=NEAR_FAR[0],
                      far_plane=NEAR_FAR[1], resolution_target=48, render_mode=6)
    lp = LightParams(light_position=(0.5, 1.5, 3.0), camera_position=(0.2, 0.5, 3.0), near_plane=NEAR_FAR[0], far_plane=NEAR_FAR[1],
                     renderer_resolution=(W, H), shadow_resolution=128)
    return W, H, p, lp


@pytest.mark.parametrize("mode", [6, 0])
def test_split_screen(conv, mode):
    from dataclasses import replace
    W, H, p, lp = split_setup(conv)
    p, lp = replace(p, render_mode=mode), replace(lp, render_mode=mode)
    plain = conv.render_frame(p, lp)
    assert (conv.render_frame(p, lp, split_screen=None) == plain).all()                  # today's frame, byte for byte
    frames = {pos: conv.render_frame(p, lp, split_screen=pos) for pos in (0.0, 0.37, 0.5, 1.0)}
    assert (conv.relight(lp) == plain).all()                                             # the splat G-buffer is untouched by the split
    mesh_planes = conv.download_mesh_gbuffer()
    conv.upload_gbuffer(mesh_planes)
    mesh_frame = conv.relight(lp)
    assert (mesh_frame != plain).any()
    for pos, frame in frames.items():
        sx = int(F(pos) * F(W))
        dx = max(0, sx - 1)
        div = [x for x in (dx, dx + 1) if x < W]
        left = [x for x in range(W) if x < sx and x not in div]
        right = [x for x in range(W) if x >= sx and x not in div]
        print(f"split {pos}: splitPixelX {sx}, divider columns {div}, {len(left)} mesh columns, {len(right)} splat columns")
        assert (frame[:, div] == 255).all()
        assert (frame[:, left] == mesh_frame[:, left]).all() and (frame[:, right] == plain[:, right]).all()


def test_split_screen_through_the_render_context(conv):
    W, H, p, lp = split_setup(conv)
    ctx = RenderContext(mcpu.three_materials())
    ctx.converter, ctx._uploaded_scene, ctx.prepassParams, ctx.lightParams = conv, ctx.scene, p, lp
    want = conv.render_frame(p, lp, split_screen=0.37)
    MeshRenderPass().execute(ctx)
    ctx.splitScreenEnabled, ctx.splitScreenPosition = True, 0.37
    GaussianRelightingPass().execute(ctx)
    assert (ctx.frame == want).all()
    ctx.splitScreenEnabled = False
    GaussianRelightingPass().execute(ctx)
    assert (ctx.frame == conv.relight(lp)).all() and (ctx.frame != want).any()


# ---- 3b. mesh against splats --------------------------------------------------------------------------------------------------------------
def _albedo_mad(splat_planes, mesh_planes):
    """Mean absolute difference (LSB) of the two albedo planes on the pixels both cover, and their number."""
    both = (splat_planes[2][..., 3] > 0) & (mesh_planes[2][..., 3] == 255)
    d = np.abs(splat_planes[2][both][:, :3].astype(np.int64) - mesh_planes[2][both][:, :3].astype(np.int64))
    return float(d.mean()), int(both.sum())


@pytest.mark.parametrize("name", ["C1 quad", "textured sphere"])
def test_mesh_against_splats(conv, name):
    """The albedo planes of the mesh G-buffer and of the splat G-buffer of the same frame (conversion at R = 256) on the pixels both
    cover: their mean absolute difference equals, within 1 LSB, the same figure from the two numpy restatements (tests/splat_ref.py
    over the same sorted quads, tests/meshrender_ref.py) — the two passes share orientation, camera and colour conventions.  The frame
    is 24 x 16 pixels: the splat restatement visits every (quad, pixel) pair."""
    import splat_ref as sr
    from mesh2splat_amd.splat import SplatParams
    W, H, R = 24, 16, 256
    if name == "C1 quad":
        scene, eye, at = synth.unit_quad(synth.procedural_textures(64, 9)), (0.6, 0.45, 1.5), (0.5, 0.5, 0.0)
    else:
        scene, eye, at = synth.cube_sphere(4, tex_size=64), (0.5, 0.4, 2.6), (0.0, 0.0, 0.0)
    proj, view = camera.perspective(50.0, W / H, *NEAR_FAR), camera.look_at(eye, at)
    conv.upload_scene(scene)
    n = conv.convert(R)
    p = PrepassParams(view_mat=view, proj_mat=proj, renderer_resolution=(W, H), near_plane=NEAR_FAR[0], far_plane=NEAR_FAR[1], resolution_target=R)
    conv.prepass(p, download=False)
    quads = conv.sort_prepass()
    splat_planes, skipped = conv.splat(SplatParams((W, H), 0))
    mesh_planes, _ = conv.mesh_render(p)
    gpu, n_gpu = _albedo_mad(splat_planes, mesh_planes)
    ref_splat, _ = sr.render(quads, W, H, 0)
    ref_mesh = rr.render(scene, proj, view, EYE, W, H, NEAR_FAR, 0)["pinned"]["planes"]
    cpu_fig, n_cpu = _albedo_mad(ref_splat, ref_mesh)
    print(f"{name}: {n} records, {len(quads)} quads; albedo mean |mesh - splats| on the GPU {gpu:.3f} LSB over {n_gpu} pixels, "
          f"restatements {cpu_fig:.3f} LSB over {n_cpu} pixels")
    assert n_gpu == n_cpu and n_gpu > W * H // 5
    assert abs(gpu - cpu_fig) <= 1.0


# ---- 4. errors and the ABI ------------------------------------------------------------------------------------------------------------------
def test_errors(hiplib):
    L = hiplib
    with Converter(0) as c:
        ok = to_c(MeshRenderParams(EYE, EYE, EYE, (64, 48)))
        assert L.m2s_device_mesh_gbuffer(c._h, 0) is None
        assert L.m2s_mesh_render(c._h, C.byref(ok), None) == 7                          # M2S_ERR_STATE: no scene
        buf = np.empty(64 * 48, np.uint64)
        assert L.m2s_download_mesh_visibility(c._h, buf.ctypes.data, buf.size) == 7
        assert L.m2s_download_mesh_gbuffer(c._h, 2, buf.ctypes.data, buf.nbytes) == 7
        c.upload_scene(Scene([mesh_of([[(-1, -1, 0), (1, -1, 0), (0, 1, 0)]])]))
        for res in ((0, 64), (64, 0), (8193, 64), (64, 8193), (-1, 64)):
            assert L.m2s_mesh_render(c._h, C.byref(to_c(MeshRenderParams(EYE, EYE, EYE, res))), None) == 1
        for mode in (-1, 7):
            assert L.m2s_mesh_render(c._h, C.byref(to_c(MeshRenderParams(EYE, EYE, EYE, (64, 48), render_mode=mode))), None) == 1
        bad = to_c(MeshRenderParams(EYE, EYE, EYE, (64, 48)))
        bad.reserved = 1
        assert L.m2s_mesh_render(c._h, C.byref(bad), None) == 1
        assert L.m2s_mesh_render(None, C.byref(ok), None) == 1 and L.m2s_mesh_render(c._h, None, None) == 1
        # split without a mesh G-buffer, then with one of another size
        from mesh2splat_amd import light as li
        lp = li.to_c(LightParams(renderer_resolution=(64, 48), shadow_resolution=16))
        c.upload_gbuffer([None, None, np.zeros((48, 64, 4), np.uint8), None, None])
        c.upload_shadow_cubemap(np.ones((6, 16, 16), F))
        assert L.m2s_relight(c._h, C.byref(lp)) == 0
        assert L.m2s_relight_split(c._h, C.byref(lp), 0.5) == 7                        # M2S_ERR_STATE
        assert L.m2s_mesh_render(c._h, C.byref(to_c(MeshRenderParams(EYE, EYE, EYE, (48, 64)))), None) == 0
        assert L.m2s_relight_split(c._h, C.byref(lp), 0.5) == 7                        # 48 x 64 is not 64 x 48
        assert L.m2s_mesh_render(c._h, C.byref(ok), None) == 0                         # out_counts may be NULL
        assert L.m2s_relight_split(c._h, C.byref(lp), 0.5) == 0
        for pos in (-0.01, 1.01, float("nan")):
            assert L.m2s_relight_split(c._h, C.byref(lp), pos) == 1
        assert L.m2s_device_mesh_gbuffer(c._h, 4) and L.m2s_device_mesh_gbuffer(c._h, 5) is None
        assert L.m2s_download_mesh_visibility(c._h, buf.ctypes.data, buf.size - 1) == 5   # M2S_ERR_CAPACITY
        assert L.m2s_download_mesh_visibility(c._h, buf.ctypes.data, buf.size) == 0 and (buf != EMPTY).any()
        v = (C.c_uint64 * 6)()
        assert L.m2s_last_mesh_render_counts(c._h, v) == 0 and v[0] == 1 and v[5] == 0
        c.set_profiling(True)
        c.mesh_render(MeshRenderParams(EYE, EYE, EYE, (640, 360)), download=False)
        assert c.last_mesh_render_ms > 0 and set(c.last_mesh_render_stage_ms()) == {"setup", "bin", "raster", "shade"}
    assert C.sizeof(MeshRenderParamsC) == 3 * 64 + 24


def test_cli_split_screen_flag(hiplib, tmp_path):
    import os
    import re
    import subprocess
    from mesh2splat_amd import gltf_io
    glb, out, png = str(tmp_path / "s.glb"), str(tmp_path / "s.ply"), str(tmp_path / "out.png")
    gltf_io.write_glb(synth.sphere_grid(2, n=5, tex_size=32), glb)
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
    r = subprocess.run([exe, glb, out, "--density", "64", "--preview-size", "160x100", "--preview", png, "--split-screen", "0.5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"split screen at 0.5: (\d+) triangles drawn \((\d+) clipped, (\d+) culled as back-facing\)", r.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(3)) > 100
    import PIL.Image
    img = np.asarray(PIL.Image.open(png).convert("RGBA"))
    assert img.shape == (100, 160, 4)
    assert (img[:, 79:81] == 255).all() and (img[:, :79] != 255).any() and (img[:, 81:] != 255).any()      # (int)(0.5 * 160) = 80: columns 79, 80
    bad = subprocess.run([exe, glb, out, "--preview", png, "--split-screen", "1.5"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2
