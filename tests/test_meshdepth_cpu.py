"""The numpy restatement of the mesh depth prepass (tests/meshdepth_ref.py — what the GPU tests hold m2s_mesh_depth to, bit for bit)
held to geometry: a float64 ray cast, ownership at shared edges, the clipper, mesh selection and orientation.  No GPU.

Achieved on the scene of test 1 (384 x 216): disagreement on hit / triangle on 0 of 82 944 pixels, max |dz_w| 6.9e-07."""
import numpy as np
import pytest

import camera
import meshdepth_ref as mr

F = np.float32
MISMATCH_CAP = 0.005        # share of pixels that may disagree on hit / miss or on the triangle (centres within ~1/256 px of an edge)
Z_TOL = 1e-5                # half the prepass's eps of 2e-5: a less accurate occluder would cull the surface it was made from


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def icosahedron(center, radius):
    t = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
                  (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)], np.float64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * radius + np.asarray(center, np.float64)
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    return v[np.array(f)].astype(F)


def quad(p00, p10, p11, p01):
    return np.array([[p00, p10, p11], [p00, p11, p01]], F)


def wall_floor_ico():
    """A wall (2 triangles), a floor (2 triangles, crossing the near plane and the left window border), an icosahedron in front of the
    wall.  No two surfaces intersect in view."""
    wall = quad((-4, 0.3, -2), (4, 0.3, -2), (4, 5, -2), (-4, 5, -2))
    floor = quad((-20, 0, 10), (6, 0, 10), (6, 0, -1.9), (-20, 0, -1.9))
    return np.concatenate([wall, floor, icosahedron((0.3, 1.0, 0.0), 0.6)])


def view_camera(res=(384, 216), eye=(0, 1.0, 4), at=(0, 0.8, 0), near=0.1, far=50.0):
    return camera.perspective(60.0, res[0] / res[1], near, far), camera.look_at(eye, at)


# ---- the float64 ray cast -----------------------------------------------------------------------------------------------------------
def ray_cast(pos, proj, view, model, W, H):
    """Pixel-centre rays against the triangles, exact geometry in float64 -> (z_w (H, W) with 1.0 = miss, triangle (H, W) or -1)."""
    PVM = (proj.astype(np.float64).T @ view.astype(np.float64).T @ model.astype(np.float64).T)       # math matrix
    inv = np.linalg.inv(PVM)
    xs = (np.arange(W) + 0.5) / W * 2 - 1
    ys = (np.arange(H) + 0.5) / H * 2 - 1
    gx, gy = np.meshgrid(xs, ys)

    def unproject(zn):
        q = np.stack([gx, gy, np.full_like(gx, zn), np.ones_like(gx)], -1) @ inv.T
        return q[..., :3] / q[..., 3:4]
    o = unproject(-1.0)
    d = unproject(1.0) - o
    best = np.ones((H, W))
    tri = np.full((H, W), -1, np.int32)
    for k, T in enumerate(np.asarray(pos, np.float64)):
        e1, e2 = T[1] - T[0], T[2] - T[0]
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(all="ignore"):
            inv_det = 1.0 / det
            tv = o - T[0]
            u = (tv * pv).sum(-1) * inv_det
            qv = np.cross(tv, e1)
            v = (d * qv).sum(-1) * inv_det
            t = qv @ e2 * inv_det
            hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)
            p = o + t[..., None] * d
            c = np.concatenate([p, np.ones_like(p[..., :1])], -1) @ PVM.T
            zw = (c[..., 2] / c[..., 3]) * 0.5 + 0.5
        win = hit & (zw < best)
        best[win] = zw[win]
        tri[win] = k
    return best, tri


def compare_with_ray_cast(pos, proj, view, model, W, H, r=None):
    r = r or mr.mesh_depth(pos, np.ones(len(pos), bool), proj, view, model, W, H)
    z, tri = ray_cast(pos, proj, view, model, W, H)
    differ = r["winner"] != tri
    share = differ.mean()
    dz = np.abs(r["image"].astype(np.float64) - z)[~differ]
    print(f"disagree {100 * share:.4f} % of {W * H} pixels, max |dz_w| {dz.max():.3e}, hit share {(tri >= 0).mean():.3f}")
    assert share <= MISMATCH_CAP
    assert dz.max() < Z_TOL
    return r, tri


# ---- 1. against geometry --------------------------------------------------------------------------------------------------------------
def test_against_ray_cast():
    pos = wall_floor_ico()
    W, H = 384, 216
    proj, view = view_camera((W, H))
    r, tri = compare_with_ray_cast(pos, proj, view, np.eye(4, dtype=F), W, H)
    assert set(np.unique(tri)) >= {0, 1, 2, 3, 4}              # wall, floor and the icosahedron are all in view
    assert (tri[:, 0] >= 2).any() and (tri[0, :] >= 2).any()   # the floor reaches the left border and the bottom row
    assert r["counts"][1] == 2 and r["counts"][2] == 0         # both floor triangles went through the clipper


def test_against_ray_cast_with_model_matrix():
    pos = wall_floor_ico()
    M = camera.trs((0.2, -0.1, 0.3), (0.2, 1, 0.1), 25.0, (1.1, 0.9, 1.2))
    proj, view = view_camera((384, 216), eye=(0.5, 1.4, 4.5))
    compare_with_ray_cast(pos, proj, view, M, 384, 216)


# ---- 2. shared edges and the top-left rule ----------------------------------------------------------------------------------------------
EYE = np.eye(4, dtype=F)


def ndc(px, W):
    """The NDC coordinate whose window coordinate is exactly px (W a power of two: every step is exact)."""
    return (np.asarray(px, np.float64) - W / 2) / (W / 2)


def screen_tris(tris_px, W, H, z=0.0):
    """(N, 3, 2) window coordinates -> (N, 3, 3) positions that identity matrices put exactly there."""
    t = np.asarray(tris_px, np.float64)
    return np.stack([ndc(t[..., 0], W), ndc(t[..., 1], H), np.full(t.shape[:-1], z)], -1).astype(F)


def fan_px():
    c = (20.5, 20.5)
    ring = [(30.5, 20.5), (28.5, 27.5), (20.5, 31.5), (13.25, 27.0), (9.5, 20.5), (12.5, 12.5), (20.5, 8.5), (27.5, 13.5)]
    return [[c, ring[i], ring[(i + 1) % 8]] for i in range(8)]


def strip_px():
    tris = []
    for j in range(4):
        for i in range(4):
            x0, y0, x1, y1 = 4.5 + 6 * i, 4.5 + 6 * j, 10.5 + 6 * i, 10.5 + 6 * j
            tris += [[(x0, y0), (x1, y0), (x1, y1)], [(x0, y0), (x1, y1), (x0, y1)]]
    return tris


@pytest.mark.parametrize("shape", ["fan", "strip"])
def test_every_pixel_owned_once(shape):
    W = H = 64
    px = fan_px() if shape == "fan" else strip_px()
    pos = screen_tris(px, W, H)
    r = mr.mesh_depth(pos, np.ones(len(pos), bool), EYE, EYE, EYE, W, H)
    assert r["frags"].max() == 1
    if shape == "fan":
        assert r["frags"][20, 20] == 1                            # the fan's centre lies on a pixel centre: one owner
        assert r["frags"].sum() > 300
    else:
        assert (r["frags"][5:28, 5:28] == 1).all()                # every centre strictly inside, the ones on shared edges included
        assert r["frags"].sum() == 24 * 24                        # top-left: the left column and the bottom row are in, the others out
        assert (r["frags"][4, 4:28] == 1).all() and (r["frags"][4:28, 4] == 1).all() and r["frags"][28].sum() == 0
    flipped = mr.mesh_depth(pos[:, ::-1], np.ones(len(pos), bool), EYE, EYE, EYE, W, H)
    assert (flipped["image"].view(np.uint32) == r["image"].view(np.uint32)).all() and (flipped["frags"] == r["frags"]).all()
    assert (np.abs(r["image"][r["frags"] == 1] - F(0.5)) < 1e-6).all() and (r["image"][r["frags"] == 0] == F(1.0)).all()


# ---- 3. near-clipped and guard-clipped triangles ----------------------------------------------------------------------------------------
def test_one_and_two_vertices_behind_the_camera():
    W, H = 384, 216
    proj, view = view_camera((W, H))
    one = np.array([[(-1.0, 0.2, -1.0), (1.5, 0.4, -1.5), (0.2, 0.9, 6.0)]], F)            # camera at z = 4: the last vertex is behind it
    two = np.array([[(0.1, 0.5, -3.0), (-2.0, 0.2, 7.0), (2.5, 1.6, 5.0)]], F)
    for pos in (one, two, np.concatenate([two, one])):
        r, tri = compare_with_ray_cast(pos, proj, view, EYE, W, H)
        assert r["counts"][0] == len(pos) and r["counts"][1] == len(pos)
        assert (tri >= 0).mean() > 0.02


def test_vertex_beyond_the_guard_band():
    W, H = 384, 216
    proj, view = view_camera((W, H))
    pos = np.array([[(-3000.0, -20.0, -5.0), (3000.0, -20.0, -5.0), (0.0, 40.0, -5.0)]], F)
    c = mr.clip_positions(mr.pvm(proj, view, EYE), pos)[0]
    assert (np.abs(c[:, 0] / c[:, 3]) * W / 2 > 16384).any()            # it would not survive the snap unclipped
    r, tri = compare_with_ray_cast(pos, proj, view, EYE, W, H)
    assert (tri == 0).all() and r["counts"][:3] == [1, 1, 0]


def test_beyond_the_far_plane_and_non_finite():
    W, H = 96, 64
    proj, view = view_camera((W, H), far=20.0)
    far_tri = np.array([[(-5, -5, -30.0), (5, -5, -30.0), (0, 5, -40.0)]], F)
    r = mr.mesh_depth(far_tri, [True], proj, view, EYE, W, H)
    assert (r["image"] == F(1.0)).all() and r["counts"][0] == 0 and r["frags"].sum() == 0
    good = np.array([[(-1, 0, 0.0), (1, 0, 0.0), (0, 2, 0.0)]], F)
    want = mr.mesh_depth(good, [True], proj, view, EYE, W, H)
    for bad in (np.nan, np.inf, -np.inf):
        b = good.copy()
        b[0, 1, 0] = bad
        r = mr.mesh_depth(np.concatenate([b, good]), [True, True], proj, view, EYE, W, H)
        assert r["counts"][:3] == [1, 0, 1]
        assert (r["image"].view(np.uint32) == want["image"].view(np.uint32)).all()


# ---- 4. mesh selection and orientation --------------------------------------------------------------------------------------------------
def test_mesh_selection():
    from mesh2splat_amd.scene import Mesh, Scene
    W, H = 96, 64
    proj, view = view_camera((W, H))

    def mesh(tris, alpha):
        v = np.zeros((len(tris) * 3, 12), F)
        v[:, 0:3] = tris.reshape(-1, 3)
        return Mesh("m", v, base_color=(1, 1, 1, alpha))
    a = np.array([[(-1, 0.2, 0.0), (1, 0.2, 0.0), (0, 2, 0.0)]], F)
    b = np.array([[(-2, 0.1, 1.0), (0, 0.1, 1.0), (-1, 1.5, 1.0)]], F)
    pos, opaque = mr.scene_triangles(Scene([mesh(a, 1.0), mesh(b, 0.999)]))
    assert opaque.tolist() == [True, False]
    r = mr.mesh_depth(pos, opaque, proj, view, EYE, W, H)
    only_a = mr.mesh_depth(a, [True], proj, view, EYE, W, H)
    assert (r["image"].view(np.uint32) == only_a["image"].view(np.uint32)).all() and (r["winner"] <= 0).all() and (r["winner"] == 0).any()
    none = mr.mesh_depth(pos, [False, False], proj, view, EYE, W, H)
    assert (none["image"] == F(1.0)).all() and none["counts"] == [0, 0, 0, 0]
    empty = mr.mesh_depth(np.zeros((0, 3, 3), F), [], proj, view, EYE, W, H)
    assert (empty["image"] == F(1.0)).all()


def edge_distance_px(p, tri, proj, view, W, H):
    """Window-space distance (pixels) from the projection of p to the nearest edge of the projected triangle; float64."""
    PV = proj.astype(np.float64).T @ view.astype(np.float64).T

    def win(q):
        c = PV @ np.append(np.asarray(q, np.float64), 1.0)
        return np.array([(c[0] / c[3] * 0.5 + 0.5) * W, (c[1] / c[3] * 0.5 + 0.5) * H])
    q, v = win(p), [win(x) for x in tri]
    d = []
    for i in range(3):
        a, b = v[i], v[(i + 1) % 3]
        e = b - a
        d.append(abs(e[0] * (q[1] - a[1]) - e[1] * (q[0] - a[0])) / max(np.hypot(*e), 1e-30))
    return min(d)


def test_orientation_and_the_prepass_lookup():
    W, H = 384, 216
    proj, view = view_camera((W, H))
    pos = wall_floor_ico()
    r = mr.mesh_depth(pos, np.ones(len(pos), bool), proj, view, EYE, W, H)
    # row 0 = bottom: the floor (below the camera) owns the bottom rows, the wall the top ones
    assert (r["winner"][0] >= 2).all() and (r["winner"][0] <= 3).all()
    top = r["winner"][H - 1]
    assert (top <= 1).all() and (top >= 0).sum() > W // 2        # (the wall is narrower than the view: background beside it)
    # a point on a triangle lands, by the prepass's own transform and uv -> GL_NEAREST rule, on a texel that triangle owns
    rng = np.random.default_rng(4)
    checked = 0
    for t in range(len(pos)):
        for _ in range(20):
            w = 0.2 + 0.4 * rng.dirichlet((1, 1, 1))                                # well inside: several texels from every edge
            p = (w[:, None] * pos[t].astype(np.float64)).sum(0).astype(F)
            ws = mr.clip_positions(EYE, p)
            vs = mr.clip_positions(view, ws[:3])
            c = (proj[0] * vs[0] + proj[1] * vs[1]) + (proj[2] * vs[2] + proj[3] * vs[3])
            if not (c[3] > 0 and abs(c[0]) < c[3] and abs(c[1]) < c[3] and abs(c[2]) < c[3]):      # outside the frustum: not drawn
                continue
            if edge_distance_px(p, pos[t], proj, view, W, H) < 1.5:                # a face seen edge-on: the texel may lie beside it
                continue
            uv = ((c[0] / c[3]) * F(0.5) + F(0.5), (c[1] / c[3]) * F(0.5) + F(0.5))
            x, y = mr.prepass_texel(uv, W, H)
            my_depth = (c[2] / c[3]) * F(0.5) + F(0.5)
            if r["winner"][y, x] == t:
                checked += 1
                assert abs(float(my_depth) - float(r["image"][y, x])) < 0.02      # the same surface (its slope across one texel)
            else:                                                                   # hidden behind a nearer surface
                assert r["image"][y, x] < my_depth
    assert checked > 100
