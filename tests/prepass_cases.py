"""Shared inputs of the prepass tests (reference pin, golden generator, GPU parity): deterministic records and a list of
named parameter sets covering every branch of gaussianSplattingPrepassCS.glsl."""
import numpy as np

import camera
from mesh2splat_amd import synth
from mesh2splat_amd.prepass import PrepassParams

SEED = 0x4D32535F50524550


def base_records(oracle, n: int = 12, R: int = 48) -> np.ndarray:
    """Records of a real conversion (textured cube-sphere) -> realistic scales / rotations / normals / pbr."""
    scene = synth.cube_sphere(n, tex_size=32)
    _, rec, _ = oracle.convert(scene, R, cap=0)
    return np.ascontiguousarray(rec, np.float32).reshape(-1, 24)


def hostile_records(n: int = 512) -> np.ndarray:
    """Random records with the things a loaded .ply can contain: translucent alpha, unnormalised quaternions, equal and
    zero scales, huge scales, positions behind and far outside the frustum, non-finite values."""
    rng = np.random.default_rng(SEED)
    r = np.zeros((n, 24), np.float32)
    r[:, 0:3] = rng.uniform(-3, 3, (n, 3))
    r[:, 3] = 1
    r[:, 4:8] = rng.uniform(0, 1, (n, 4))
    r[:, 8:11] = np.exp(rng.uniform(-9, 1, (n, 3)))
    r[:, 12:15] = rng.normal(size=(n, 3))
    r[:, 16:20] = rng.normal(size=(n, 4))
    r[:, 20:22] = rng.uniform(0, 1, (n, 2))
    r[:, 23] = 1
    r[::7, 8:11] = r[::7, 8:9]                     # equal scales (min-index ties, format 1)
    r[5::31, 8:11] = 0                             # degenerate
    r[9::37, 8:11] = 1e4                           # quad axes hit the 1024 px clamp
    r[11::41, 16:20] = 0                           # zero quaternion
    r[3::53, 0:3] = np.nan
    r[4::59, 0:3] = np.inf
    r[6::61, 8] = np.nan
    r[::2, 7] = 1.0                                # opaque half (depth test applies at alpha > .95)
    return r


def needle_records(n, seed=11):
    """Needle-shaped Gaussians in front of the default camera: one scale 10^4..10^6 times the others, random orientation.  Their
    screen-space covariance is numerically rank 1, so lambda2 = (mid - delta) / 2 is pure rounding noise and comes out negative
    for part of them — the shader's LAST cull test (gaussianSplattingPrepassCS.glsl:183) then removes them."""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 24), np.float32)
    r[:, 0:3] = rng.uniform(-0.6, 0.6, (n, 3))
    r[:, 3] = 1
    r[:, 4:8] = rng.uniform(0.2, 1, (n, 4))
    r[:, 8] = np.exp(rng.uniform(np.log(3e2), np.log(3e4), n))
    r[:, 9:11] = 1e-2
    q = rng.normal(size=(n, 4))
    r[:, 16:20] = q / np.linalg.norm(q, axis=1, keepdims=True)
    r[:, 12:15] = (0, 0, 1)
    r[:, 20:22] = 0.5
    r[:, 23] = 1
    return r


def last_test_culls(oracle, p, rec) -> np.ndarray:
    """Indices of the records that ONLY the shader's last test (lambda2 < 0) removes at `p`: they survive the oracle's prepass with their
    scale and rotation replaced by 1e-3 and the identity (a small sphere: every earlier test — frustum, depth image — sees the same
    position and alpha), and do not survive it with their own."""
    return np.setdiff1d(surviving_records(oracle, p, _as_balls(rec)), surviving_records(oracle, p, rec))


def _as_balls(rec) -> np.ndarray:
    ball = np.array(rec, np.float32).reshape(-1, 24)
    ball[:, 8:11] = 1e-3
    ball[:, 16:20] = (1, 0, 0, 0)                  # (castQuatToMat3 reads x as the scalar part)
    return ball


def sorted_with_sources(oracle, p, rec):
    """-> (quads, sources): the oracle's prepass of `rec` at `p` under numpy's stable argsort of the depth bits — what m2s_prepass +
    m2s_sort_prepass and m2s_prepass_sorted leave in the sorted-quads buffer — and the record index of every one of those quads."""
    rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 24)
    k, q, d = oracle.prepass(p, rec)
    order = np.argsort(d.view(np.uint32), kind="stable")
    return q[order], surviving_records(oracle, p, rec)[order].astype(np.uint32)


def passing_the_early_tests_by_depth(oracle, p, rec) -> np.ndarray:
    """Indices of the records that pass every test but the last at `p`, in the order m2s_prepass_sorted's depth sort gives them (the
    depth is a function of the position alone: the oracle's, of the same records as small spheres)."""
    ball = _as_balls(rec)
    idx = surviving_records(oracle, p, ball)
    _, _, d = oracle.prepass(p, ball)
    return idx[np.argsort(d.view(np.uint32), kind="stable")]


def surviving_records(oracle, p, rec) -> np.ndarray:
    """Indices of the records that survive the oracle's prepass at `p`, ascending.  The prepass copies a record's metallic factor into its
    quad untouched (pbr.x -> normal.w, float 19) and no test reads it: a copy of the records carries the record index there."""
    tagged = np.array(rec, np.float32).reshape(-1, 24)
    assert tagged.shape[0] < 1 << 24               # (every index is a float32)
    tagged[:, 20] = np.arange(tagged.shape[0], dtype=np.float32)
    k, q, _ = oracle.prepass(p, tagged)
    idx = q[:, 19].astype(np.int64)
    assert idx.size == k and (np.diff(idx) > 0).all()
    return idx


def mixed_records(oracle) -> np.ndarray:
    """Ordinary records, hostile ones, needles (in the middle) and the first 3000 rows again: equal keys exercise the sort's stability."""
    rec = np.concatenate([base_records(oracle, 14, 64), hostile_records(2048), needle_records(2000)])
    return np.concatenate([rec, rec[:3000]])


def default_camera(res=(640, 360)):
    view = camera.look_at((1.6, 1.1, 2.3), (0.1, 0.0, -0.1))
    proj = camera.perspective(45.0, res[0] / res[1], 0.01, 100.0)
    return view, proj


def second_frame(p):
    """`p` seen by the second camera of the m2s_prepass_sorted tests: 800 x 450, a model matrix with rotation + non-uniform scale +
    translation (column-major: rows = columns)."""
    from dataclasses import replace
    view, proj = default_camera((800, 450))
    model = np.array([[0.0, 1.3, 0.0, 0.0], [-0.7, 0.0, 0.0, 0.0], [0.0, 0.0, 1.1, 0.0], [0.05, -0.1, 0.2, 1.0]], np.float32)
    return replace(p, view_mat=view, proj_mat=proj, model_mat=model, renderer_resolution=(800, 450))


def orbit_views(R: int = 64):
    """The six orbit views of the prune tests around cube_sphere(8): 128 x 128, three azimuths at elevations 0 and 40 degrees."""
    from mesh2splat_amd.prune import orbit_cameras
    return [cam.frame_params(R, (0, 0, 0), 0.0)[0] for cam in orbit_cameras(synth.cube_sphere(8), 3, 128, 128, (0, 40))]


def depth_image(res, seed=3) -> np.ndarray:
    """Window-space depth with structure on the scale of the splats: some occlude, some do not."""
    rng = np.random.default_rng(seed)
    h, w = res[1] // 4, res[0] // 4
    coarse = rng.uniform(0.97, 1.0, (h // 8 + 1, w // 8 + 1)).astype(np.float32)
    d = np.kron(coarse, np.ones((8, 8), np.float32))[:h, :w]
    return np.ascontiguousarray(d)


def cases():
    """-> list of (name, PrepassParams)"""
    res = (640, 360)
    view, proj = default_camera(res)
    out = []

    def add(name, **kw):
        p = PrepassParams(view_mat=view, proj_mat=proj, renderer_resolution=res, resolution_target=48, **kw)
        out.append((name, p))

    add("colour")                                                       # format 0, mode 0, identity model
    add("depth_mode", render_mode=1)
    add("normal_mode", render_mode=2)
    add("geometry_mode", render_mode=3)
    add("mode6", render_mode=6)
    add("mode4_black", render_mode=4)
    add("ply_classic", format=1, render_mode=2)                        # shortest-axis normal
    add("ply_classic_pbr", format=1, ply_has_pbr=True, render_mode=2)
    add("ply_compressed", format=2, render_mode=2)                     # normal stays (1,0,0,0)
    add("format3", format=3, gaussian_std=0.9)
    add("depth_test", perform_mesh_depth_test=True, mesh_depth=depth_image(res))
    add("depth_test_format1_ignored", perform_mesh_depth_test=True, mesh_depth=depth_image(res), format=1)
    add("model_trs", model_mat=camera.trs((0.3, -0.2, 0.1), (1, 2, 3), 37.0, (1.5, 0.7, 1.2)), render_mode=2)
    add("wide_std", gaussian_std=4.0)
    # camera inside the object looking out: many behind the eye, near-plane culls
    p = PrepassParams(view_mat=camera.look_at((0.2, 0.1, 0.0), (1, 0.3, 0.2)), proj_mat=camera.perspective(70.0, 1.0, 0.01, 100.0),
                      renderer_resolution=(512, 512), resolution_target=48)
    out.append(("inside", p))
    return out
