"""The numpy restatement of the mesh render pass (tests/meshrender_ref.py — what the GPU tests hold m2s_mesh_render to) held to
geometry: a float64 ray cast with back-face culling, perspective-correct interpolation, draw order, ownership at shared edges.  It
also defines the scenes of tests/test_gpu_meshrender.py and holds their ill-conditioned share here, without a GPU.

Achieved (384 x 216, wall + clipped floor + icosahedron): winner disagrees with the ray cast on 0 of 82 944 pixels (1 with a model
matrix), position within 1.6e-6 of the hit point; ill-conditioned share of the GPU scenes 0 %."""
import numpy as np
import pytest

import camera
import meshrender_ref as rr
import test_meshdepth_cpu as cpu
from mesh2splat_amd import synth
from mesh2splat_amd.scene import Mesh, Scene

F = np.float32
EYE = np.eye(4, dtype=F)
MISMATCH_CAP = 0.005        # the cap of the depth test: centres within ~1/256 px of an edge
ILL_CAP = 0.005             # share of pixels on which the pinned and the float64 evaluation differ by more than one output step
NEAR_FAR = (0.1, 50.0)


def mesh_of(tris, alpha=1.0, name="m", color=(0.7, 0.6, 0.5), textures=None, uv=None):
    """Triangles (N, 3, 3) -> a Mesh with flat normals, a tangent along the first edge and (optionally) per-vertex UVs (N, 3, 2)."""
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    v = np.zeros((len(tris) * 3, 12), F)
    v[:, 0:3] = tris.reshape(-1, 3)
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    n = np.cross(e1, e2).astype(np.float64)
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    t = e1 / np.maximum(np.linalg.norm(e1, axis=1, keepdims=True), 1e-30)
    v[:, 3:6] = np.repeat(n, 3, 0)
    v[:, 6:9] = np.repeat(t, 3, 0)
    v[:, 9] = 1
    if uv is not None:
        v[:, 10:12] = np.asarray(uv, F).reshape(-1, 2)
    return Mesh(name, v, base_color=(*color, alpha), textures=dict(textures or {}))


# ---- the float64 ray cast with GL_CULL_FACE -----------------------------------------------------------------------------------------------
def ray_cast(pos, proj, view, model, W, H):
    """Pixel-centre rays against the front faces (CCW seen from the eye), float64 -> (triangle (H, W) or -1, world hit point (H, W, 3))."""
    Mm = model.astype(np.float64).T
    PV = proj.astype(np.float64).T @ view.astype(np.float64).T
    inv = np.linalg.inv(PV)
    gx, gy = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)

    def unproject(zn):
        q = np.stack([gx, gy, np.full_like(gx, zn), np.ones_like(gx)], -1) @ inv.T
        return q[..., :3] / q[..., 3:4]
    o = unproject(-1.0)
    d = unproject(1.0) - o
    best = np.ones((H, W))
    tri = np.full((H, W), -1, np.int64)
    hitp = np.zeros((H, W, 3))
    world = np.concatenate([np.asarray(pos, np.float64), np.ones((len(pos), 3, 1))], -1) @ Mm.T
    for k, T4 in enumerate(world):
        T = T4[:, :3]
        e1, e2 = T[1] - T[0], T[2] - T[0]
        pv = np.cross(d, e2)
        det = pv @ e1                                              # = -d . (e1 x e2): positive when the face looks at the eye
        with np.errstate(all="ignore"):
            inv_det = 1.0 / det
            tv = o - T[0]
            u = (tv * pv).sum(-1) * inv_det
            qv = np.cross(tv, e1)
            v = (d * qv).sum(-1) * inv_det
            t = qv @ e2 * inv_det
            hit = (det > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)
            p = o + t[..., None] * d
            c = np.concatenate([p, np.ones_like(p[..., :1])], -1) @ PV.T
            zw = (c[..., 2] / c[..., 3]) * 0.5 + 0.5
        win = hit & (zw < best)
        best[win] = zw[win]
        tri[win] = k
        hitp[win] = p[win]
    return tri, hitp


# ---- 1. winner and position against geometry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_model", [False, True])
def test_winner_and_position_against_ray_cast(with_model):
    W, H = 384, 216
    pos = cpu.wall_floor_ico()
    if with_model:
        model = camera.trs((0.2, -0.1, 0.3), (0.2, 1, 0.1), 25.0, (1.1, 0.9, 1.2))
        proj, view = cpu.view_camera((W, H), eye=(0.5, 1.4, 4.5))
    else:
        model = EYE
        proj, view = cpu.view_camera((W, H))
    scene = Scene([mesh_of(pos)])
    v = rr.visibility(pos, proj, view, model, W, H)
    tri, hitp = ray_cast(pos, proj, view, model, W, H)
    differ = v["winner"] != tri
    print(f"winner disagrees on {differ.sum()} of {W * H} pixels; counts {v['counts']}")
    assert differ.mean() <= MISMATCH_CAP
    assert v["counts"][1] == 2 and v["counts"][4] >= 8            # the floor is clipped; the icosahedron's far side is culled
    s = rr.shade(rr.scene_arrays(scene), v["winner"], proj, view, model, W, H, NEAR_FAR, 0, F)
    same = ~differ & (tri >= 0)
    err = np.abs(s["raw"]["pos"] - hitp)[same].max()
    print(f"position before half rounding: max |error| {err:.2e}")
    assert err < 1e-5
    # the depth of the winner is the depth pass's: same bits wherever that pass (no culling) sees the same triangle
    import meshdepth_ref as md
    d = md.mesh_depth(pos, np.ones(len(pos), bool), proj, view, model, W, H)
    agree = d["winner"] == v["winner"]
    assert agree.mean() > 0.99 and (d["image"].view(np.uint32) == v["depth"].view(np.uint32))[agree].all()


# ---- 2. perspective-correct interpolation ----------------------------------------------------------------------------------------------------
def oblique_quad(textures=None):
    """A 4 x 3 quad in the plane y = 0 whose UV is affine in world position, seen at a grazing angle."""
    c = np.array([(-2, 0, -4), (2, 0, -4), (2, 0, 2), (-2, 0, 2)], F)
    tris = np.array([[c[3], c[2], c[1]], [c[3], c[1], c[0]]], F)        # CCW seen from above
    uv = np.stack([tris[..., 0] * 0.25 + 0.5, tris[..., 2] * -0.125 + 0.25], -1)
    return Scene([mesh_of(tris, uv=uv, textures=textures)])


def oblique_camera(W, H):
    return camera.perspective(55.0, W / H, *NEAR_FAR), camera.look_at((0.3, 0.7, 3.2), (0, 0, -1.0))


def test_uv_is_perspective_correct():
    W, H = 192, 108
    scene = oblique_quad()
    proj, view = oblique_camera(W, H)
    arr = rr.scene_arrays(scene)
    v = rr.visibility(arr["pos"], proj, view, EYE, W, H)
    assert (v["winner"] >= 0).mean() > 0.2
    s = rr.shade(arr, v["winner"], proj, view, EYE, W, H, NEAR_FAR, 0, F)
    hit = v["winner"] >= 0
    p, uv, lam = s["raw"]["pos"][hit], s["raw"]["uv"][hit], s["raw"]["lam"][hit]
    want = np.stack([p[:, 0] * 0.25 + 0.5, p[:, 2] * -0.125 + 0.25], -1)
    tri, hitp = ray_cast(arr["pos"], proj, view, EYE, W, H)
    truth = hitp[hit]
    print(f"uv against the affine map of the interpolated position {np.abs(uv - want).max():.2e}, of the ray's hit point "
          f"{np.abs(uv - np.stack([truth[:, 0] * 0.25 + 0.5, truth[:, 2] * -0.125 + 0.25], -1))[tri[hit] >= 0].max():.2e}")
    assert np.abs(uv - np.stack([truth[:, 0] * 0.25 + 0.5, truth[:, 2] * -0.125 + 0.25], -1))[tri[hit] >= 0].max() < 1e-5
    # screen-linear interpolation of the same corners misses by far more: the test can tell the two apart
    PVM = rr.md.pvm(proj, view, EYE)
    c = rr.md.clip_positions(PVM, arr["pos"][v["winner"][hit]]).astype(np.float64)
    w = lam * c[..., 3]                                               # lambda_i w_i ~ screen-space barycentrics (unnormalised)
    lin = w / w.sum(1, keepdims=True)
    uv_lin = (lin[..., None] * arr["uv"][v["winner"][hit]]).sum(1)
    assert np.abs(uv_lin - want).max() > 0.05


# ---- 3. culling, draw order, translucency ------------------------------------------------------------------------------------------------------
def test_reversed_winding_draws_nothing_and_a_closed_solid_shows_front_faces_only():
    W, H = 96, 64
    proj, view = cpu.view_camera((W, H))
    tri = np.array([[(-1, 0.2, 0.0), (1, 0.2, 0.0), (0, 2, 0.0)]], F)
    front = rr.visibility(tri, proj, view, EYE, W, H)
    back = rr.visibility(tri[:, ::-1], proj, view, EYE, W, H)
    assert (front["winner"] == 0).sum() > 100 and front["counts"] == [1, 0, 0, front["counts"][3], 0]
    assert (back["winner"] == -1).all() and (back["vis"] == rr.EMPTY).all() and back["counts"][0] == 0 and back["counts"][4] == 1
    ico = cpu.icosahedron((0.1, 0.9, 0.0), 0.8)
    v = rr.visibility(ico, proj, view, EYE, W, H)
    eye = np.array([0, 1.0, 4.0])
    n = np.cross(ico[:, 1] - ico[:, 0], ico[:, 2] - ico[:, 0]).astype(np.float64)
    facing = ((eye - ico[:, 0].astype(np.float64)) * n).sum(1) > 0
    assert 0 < facing.sum() < 20
    assert set(np.unique(v["winner"])) - {-1} <= set(np.nonzero(facing)[0])
    assert v["frags"].max() == 1                                       # a convex solid: one front face per pixel
    assert v["counts"][0] + v["counts"][4] == 20


def test_coincident_triangles_the_lower_index_wins():
    W, H = 96, 64
    proj, view = cpu.view_camera((W, H))
    tri = np.array([(-1, 0.2, 0.0), (1, 0.2, 0.0), (0, 2, 0.0)], F)
    v = rr.visibility(np.stack([tri, tri, tri[[1, 2, 0]]]), proj, view, EYE, W, H)
    assert (v["frags"][v["winner"] >= 0] == 3).all() and set(np.unique(v["winner"])) == {-1, 0}
    first = rr.visibility(tri[None], proj, view, EYE, W, H, tri_first=5)
    assert ((first["vis"] & np.uint64(0xFFFFFFFF))[first["winner"] >= 0] == 5).all()     # the index in the key is global


def test_a_translucent_mesh_is_drawn():
    W, H = 96, 64
    proj, view = cpu.view_camera((W, H))
    a = np.array([[(-1, 0.2, 0.0), (1, 0.2, 0.0), (0, 2, 0.0)]], F)
    scene = Scene([mesh_of(a, alpha=0.4, color=(0.2, 0.4, 0.8))])
    r = rr.render(scene, proj, view, EYE, W, H)
    hit = r["vis"]["winner"] == 0
    assert hit.sum() > 100
    assert (r["pinned"]["planes"][2][hit] == (51, 102, 204, 255)).all() and (r["pinned"]["planes"][2][~hit] == 0).all()
    assert (r["pinned"]["planes"][4][hit] == (26, 128, 0, 255)).all()                    # the defaults (0.1, 0.5)
    for k in (0, 1, 3):
        assert (r["pinned"]["planes"][k][~hit] == 0).all() and (r["pinned"]["planes"][k][hit][:, 3] == 1).all()


@pytest.mark.parametrize("shape", ["fan", "strip"])
def test_every_pixel_owned_once(shape):
    W = H = 64
    pos = cpu.screen_tris(cpu.fan_px() if shape == "fan" else cpu.strip_px(), W, H)
    v = rr.visibility(pos, EYE, EYE, EYE, W, H)
    assert v["frags"].max() == 1 and v["counts"][4] == 0
    assert v["frags"].sum() == 24 * 24 if shape == "strip" else v["frags"].sum() > 300
    assert ((v["winner"] >= 0) == (v["frags"] == 1)).all()
    assert rr.visibility(pos[:, ::-1], EYE, EYE, EYE, W, H)["frags"].sum() == 0


# ---- 4. the scenes of the GPU tests, and their ill-conditioned share ---------------------------------------------------------------------------
def sphere_scene(n=5, tex=64):
    return synth.cube_sphere(n, tex_size=tex)


def three_materials():
    tex = synth.procedural_textures(64, 11)
    small = synth.procedural_textures(32, 5)
    return Scene([Mesh("all", synth.cube_sphere_vertices(3, 0.45, (-1.0, 0, 0)), base_color=(0.9, 0.8, 1.0, 1.0), textures=tex),
                  Mesh("albedo", synth.cube_sphere_vertices(3, 0.45, (0.0, 0, 0)), base_color=(1.0, 0.7, 0.6, 0.5),
                       textures={"baseColorTexture": small["baseColorTexture"]}),
                  Mesh("none", synth.cube_sphere_vertices(3, 0.45, (1.0, 0, 0)), base_color=(0.3, 0.6, 0.9, 1.0))])


def gpu_plane_cases():
    """name -> (scene, proj, view, model, W, H, render mode): every scene whose planes the GPU tests compare."""
    W, H = 97, 61
    proj = camera.perspective(50.0, W / H, *NEAR_FAR)
    cases = {
        "sphere close": (sphere_scene(), proj, camera.look_at((0.5, 0.4, 1.7), (0, 0, 0)), EYE, W, H, 0),
        "sphere far": (sphere_scene(), proj, camera.look_at((3.0, 5.0, 44.0), (0, 0, 0)), EYE, W, H, 0),
        "oblique quad": (oblique_quad(synth.procedural_textures(64, 3)), *oblique_camera(W, H), EYE, W, H, 0),
    }
    model = camera.trs((0.1, -0.05, 0.2), (0.3, 1, 0.2), 20.0, (1.1, 0.9, 1.0))
    view3 = camera.look_at((0.2, 0.5, 3.0), (0, 0, 0))
    for mode in range(7):
        cases[f"three materials, mode {mode}"] = (three_materials(), proj, view3, model, W, H, mode)
    return cases


_REF = {}


def reference(name):
    """The restatement of one GPU case, computed once per session and shared (the GPU tests read it, nothing changes it)."""
    if name not in _REF:
        scene, proj, view, model, W, H, mode = gpu_plane_cases()[name]
        _REF[name] = rr.render(scene, proj, view, model, W, H, NEAR_FAR, mode)
    return _REF[name]


@pytest.mark.parametrize("name", list(gpu_plane_cases()))
def test_ill_conditioned_share_of_the_gpu_scenes(name):
    r = reference(name)
    hit = r["vis"]["winner"] >= 0
    ill = ~r["well"]
    lod = r["pinned"]["raw"]["lod"][hit]
    print(f"{name}: {hit.sum()} covered pixels, ill-conditioned {ill.sum()} ({100 * ill.mean():.3f} %), "
          f"lod {np.nanmin(lod) if np.isfinite(lod).any() else float('nan'):.2f} .. {np.nanmax(lod) if np.isfinite(lod).any() else float('nan'):.2f}")
    assert hit.sum() >= 8
    assert ill.mean() <= ILL_CAP
    if name == "sphere close":
        assert (lod <= 0).mean() > 0.5 and (lod > 0).any()             # magnification on most pixels, two-level blends towards the rim
    if name == "sphere far":
        assert (lod >= 4).any() and (lod < 4).any()                    # the clamp to the last level, and the blend below it
