"""-m gpu: the shadow pass (m2s_shadow, k_shadow_*) and the relighting pass (m2s_relight, k_relight) through the C ABI against the
numpy restatement tests/light_ref.py.  Quad lists and cubes: bit-identical.  Shadow counts: exactly equal.  Lit colour bytes: within
U8_TOL on every well-conditioned pixel (light_ref.relight says which are not; at most 0.5 % per case, asserted by the CPU test)."""
import numpy as np
import pytest

import camera
import light_ref as lr
from mesh2splat_amd import _lib, synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prepass import PrepassParams

pytestmark = pytest.mark.gpu
U8_TOL = 1            # unorm8 LSB, the bound tests/test_gpu_splat.py uses


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def same_bits(a, b):
    """The standard tests/test_gpu_prepass.py holds the viewer prepass to: equal bits, or NaN in both (IEEE leaves a NaN's sign and payload open)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def light_params(lp: lr.Light, res, S, mode=6, counts=True) -> LightParams:
    return LightParams(lp.light_position, lp.light_color, lp.light_intensity, lp.camera_position, lp.near_plane, lp.far_plane, mode,
                       tuple(res), S, counts)


def records(n, seed, spread=3.0):
    """Seeded random records around the origin, plus the hostile ones: face-tie directions, a NaN position, a record at the light,
    needles, records beyond the far plane (d >= 1), duplicates (equal depths), records close to the light (quads larger than a face)."""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 24), np.float32)
    r[:, 0:3] = rng.uniform(-spread, spread, (n, 3))
    r[:, 3] = 1
    r[:, 4:8] = rng.uniform(0, 1, (n, 4))
    r[:, 8:10] = rng.uniform(0.002, 0.08, (n, 2))
    r[:, 10] = 1e-7
    q = rng.normal(size=(n, 4))
    r[:, 16:20] = q / np.linalg.norm(q, axis=1, keepdims=True)
    r[:, 12:15] = (0, 0, 1)
    r[:, 20:24] = (0.1, 0.6, 0, 1)
    return r


def hostile(r, light, to_local=None):
    """to_local: maps a world position to the model-space position that the model matrix sends there EXACTLY (None: identity)."""
    L = np.asarray(light, np.float32)
    r = r.copy()
    pos_before = r[:, 0:3].copy()
    r[0, 0:3] = L + np.float32([1, 1, 0]); r[1, 0:3] = L + np.float32([0, -1, -1]); r[2, 0:3] = L + np.float32([-1, 0, 1])
    r[3, 0:3] = L + np.float32([1, 1, 1]); r[4, 0:3] = (np.nan, 0, 0); r[5, 0:3] = L
    r[6, 8:11] = (5.0, 1e-7, 1e-7); r[7, 8:11] = (1e-7, 30.0, 1e-7)                   # needles
    r[8, 0:3] = L + np.float32([0, 0, -80]); r[9, 0:3] = L + np.float32([70, 1, 2])   # beyond the far plane
    r[10] = r[11]; r[12] = r[11]                                                      # equal depths
    r[13, 0:3] = L + np.float32([0.02, 0.01, -0.05]); r[13, 8:11] = 0.05              # close to the light: larger than a face
    r[14, 0:3] = L + np.float32([0.3, -0.02, 0.01]); r[14, 8:11] = 0.2
    r[15, 0:3] = (np.inf, 0, 0)
    # needles long enough for the fp32 eigenvalue difference to come out negative (positive in exact arithmetic): the lambda2 < 0 cull
    r[16:48, 8:11] = (5e3, 1e-7, 1e-7); r[48:80, 8:11] = (1e-7, 5e4, 1e-7)
    if to_local is not None:
        moved = (r[:16, 0:3].view(np.uint32) != pos_before[:16].view(np.uint32)).any(1)
        r[:16, 0:3][moved] = to_local(r[:16, 0:3][moved])
    return r


# A model matrix whose arithmetic is exact on dyadic inputs: scale (2, 0.5, 4), a quarter turn about z, translation (0.5, -0.25, 0.125):
# M p = (0.5 - 0.5 py, 2 px - 0.25, 4 pz + 0.125), so the hostile world positions (ties, at the light) are reached exactly.
EXACT_MODEL = np.array([[0, 2, 0, 0], [-0.5, 0, 0, 0], [0, 0, 4, 0], [0.5, -0.25, 0.125, 1]], np.float32)


def exact_to_local(w):
    w = np.asarray(w, np.float32)
    return np.stack([(w[:, 1] + np.float32(0.25)) / np.float32(2), (np.float32(0.5) - w[:, 0]) * np.float32(2), (w[:, 2] - np.float32(0.125)) / np.float32(4)], 1)


def pp_for(model, res, fmt=0, std=0.65, R=8):
    return PrepassParams(model_mat=model, renderer_resolution=res, near_plane=0.01, far_plane=50.0, gaussian_std=std, resolution_target=R, format=fmt)


def ref_lists(rec, pp, lp):
    return lr.shadow_quads(rec, pp.model_mat, pp.renderer_resolution, (pp.near_plane, pp.far_plane), pp.gaussian_std, pp.resolution_target,
                           pp.format, lp.light_position, (lp.near_plane, lp.far_plane))


def gpu_shadow(conv, rec, pp, lp, S, res):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rec, np.float32)).cuda()
    per_face, skipped, cube = conv.shadow(pp, light_params(lp, res, S), records=t)
    lists = [conv.download_shadow_quads(f, per_face[f]) for f in range(6)]
    return per_face, skipped, cube, lists


# ---- 1. stage A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,model", [(0, "identity"), (1, "identity"), (0, "trs"), (0, "exact")])
def test_stage_a_lists_bit_identical(conv, fmt, model):
    lp = lr.Light(pos=(0.25, -0.5, 0.75))
    M = {"identity": np.eye(4, dtype=np.float32), "trs": camera.trs((0.3, -0.2, 0.1), (1, 2, 3), 37.0, (1.5, 0.75, 1.25)), "exact": EXACT_MODEL}[model]
    # ("trs": an arbitrary rotation cannot place a record exactly on a tie direction; there the hostile records sit away from the light)
    rec = hostile(records(5000, 5 + fmt), (9, 9, 9) if model == "trs" else lp.light_position, exact_to_local if model == "exact" else None)
    pp = pp_for(M, (320, 200), fmt)
    per_face, skipped, cube, lists = gpu_shadow(conv, rec, pp, lp, 64, (320, 200))
    want, (face, clip_ok, lam_ok) = lr.shadow_quads(rec, pp.model_mat, pp.renderer_resolution, (pp.near_plane, pp.far_plane), pp.gaussian_std,
                                                    pp.resolution_target, pp.format, lp.light_position, (lp.near_plane, lp.far_plane), masks=True)
    # the cases are what they claim to be, on the restatement: needles culled by the lambda2 test ALONE, records culled by the 1.05 w test,
    # and (without an inexact model matrix) the tie directions on the faces the `if` chain gives them, the NaN and at-the-light ones on face 5
    assert (clip_ok[16:80] & ~lam_ok[16:80]).sum() >= 5, "no needle fails only the lambda2 test"
    if model != "trs":
        assert (~clip_ok).any()
        with np.errstate(all="ignore"):
            ws = (rec[:6, 0:3] @ M[:3, :3] + M[3, :3]).astype(np.float32)
        assert np.array_equal(ws[[0, 1, 2, 3, 5]], (np.float32(lp.light_position) + np.float32([[1, 1, 0], [0, -1, -1], [-1, 0, 1], [1, 1, 1], [0, 0, 0]])))
        assert face[:6].tolist() == [0, 3, 1, 0, 5, 5]
    assert per_face == [w.shape[0] for w in want], (per_face, [w.shape[0] for w in want])
    assert min(per_face) > 0
    assert sum(per_face) < rec.shape[0]                           # some are culled
    for f in range(6):
        assert same_bits(lists[f], want[f]), f"face {f}"
    assert conv.last_shadow_counts()["quads_per_face"] == per_face


# ---- 2. the cube -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n", [(64, 4000), (257, 3000), (1024, 1500)])
def test_cube_byte_identical(conv, S, n):
    lp = lr.Light(pos=(0.25, -0.5, 0.75))
    res = (320, 200)
    pp = pp_for(np.eye(4, dtype=np.float32), res)
    rec = hostile(records(n, 20 + S), lp.light_position)
    per_face, skipped, cube, lists = gpu_shadow(conv, rec, pp, lp, S, res)
    want, wskipped = lr.shadow_cube(ref_lists(rec, pp, lp), S, lp.light_position, lp.far_plane)
    print(f"S={S}: quads per face {per_face}, skipped {skipped}, texels below 1.0: {(want < 1).mean():.3f}, counts {conv.last_shadow_counts()}")
    assert skipped == wskipped and skipped >= 1                    # the NaN record's quad
    assert np.array_equal(cube.view(np.uint32), want.view(np.uint32)), np.argwhere(cube != want)[:5].tolist()
    assert (want < 1).any() and (want == 1).any() and want.min() >= 0
    # twice in a row: the same bytes; fewer records afterwards: no stale texel
    _, _, again, _ = gpu_shadow(conv, rec, pp, lp, S, res)
    assert np.array_equal(again.view(np.uint32), cube.view(np.uint32))
    few = rec[100:140]
    _, _, cube2, _ = gpu_shadow(conv, few, pp, lp, S, res)
    want2, _ = lr.shadow_cube(ref_lists(few, pp, lp), S, lp.light_position, lp.far_plane)
    assert np.array_equal(cube2.view(np.uint32), want2.view(np.uint32))


def window_quad(S, cx, cy, ax, ay, bx, by, depth, light, far, face_axis=2):
    """A shadow quad from window-space numbers on an S x S face: centre (cx, cy), axes (ax, ay), (bx, by) in texels; d ~ depth."""
    h = np.float32(S) * np.float32(0.5)
    q = np.zeros(12, np.float32)
    q[0], q[1] = np.float32(cx) / h - np.float32(1), np.float32(cy) / h - np.float32(1)
    q[2], q[3] = 0.5, 1
    q[4:8] = np.float32([ax, ay, bx, by]) / h
    q[8:11] = np.float32(light)
    q[8 + face_axis] += np.float32(depth * far)
    q[11] = 1
    return q


def hand_lists(S, light, far, seed):
    """Six lists of hand-placed quads: what stage A produces only by chance or not at all."""
    rng = np.random.default_rng(seed)
    T = lr.sr.TILE
    lists = []
    for fc in range(6):
        W = lambda *a, **k: window_quad(S, *a, light=light, far=far, face_axis=fc % 3, **k)
        qs = [
            # vertices exactly on texel centres (the top-left rule decides), one inside a tile, one across a tile corner
            W(8.5, 8.5, 3, 0, 0, 3, 0.30), W(T + 0.5, T + 0.5, 5, 0, 0, -5, 0.31), W(T - 0.5, 2 * T - 0.5, 0, 8, 8, 0, 0.32),
            # edges exactly on tile borders and on the face's borders
            W(T, T, T / 2, 0, 0, T / 2, 0.33), W(2 * T, T / 2, T, 0, 0, T / 2, 0.34), W(S / 2, S - 0.5, S / 2, 0, 0, 0.5, 0.35), W(S - 0.5, S / 2, 0.5, 0, 0, S / 2, 0.36),
            W(0.5, 0.5, 0.5, 0, 0, 0.5, 0.2), W(S - 0.5, S - 0.5, 0.5, 0, 0, 0.5, 0.2), W(S - 1.0, S - 1.0, 1.0, 0, 0, 1.0, 0.25),
            # zero-area: no axes, collinear axes, one axis
            W(20.5, 20.5, 0, 0, 0, 0, 0.05), W(21.5, 20.5, 3, 1, 6, 2, 0.05), W(22.5, 20.5, 4, 0, 0, 0, 0.05),
            # off-face (every side), partly off-face, off the corner
            W(-50, 10, 5, 0, 0, 5, 0.1), W(S + 40, 10, 5, 0, 0, 5, 0.1), W(10, -30, 5, 0, 0, 5, 0.1), W(10, S + 30, 5, 0, 0, 5, 0.1),
            W(0, 0, 10, 0, 0, 6, 0.4), W(S, S, 7, 2, -2, 7, 0.41), W(-3, S / 2, 6, 3, -3, 6, 0.42),
            # larger than the face; d >= 1; equal depths; a nearer one inside a farther one
            W(S / 2, S / 2, S, 0, 0, S, 0.9), W(S / 3, S / 3, 9, 0, 0, 9, 1.0), W(S / 3, S / 3, 9, 0, 0, 9, 1.5),
            W(40.25, 12.75, 6, 1, -1, 6, 0.5), W(41.25, 13.75, 6, 1, -1, 6, 0.5), W(40.25, 12.75, 2, 0, 0, 2, 0.45),
            # beyond the guard band; non-finite fields
            W(S / 2, S / 2, 40000, 0, 0, 3, 0.1), W(10, 10, np.nan, 0, 0, 3, 0.1), W(np.inf, 10, 3, 0, 0, 3, 0.1),
        ]
        nanws = W(12, 12, 3, 0, 0, 3, 0.1)
        nanws[9] = np.nan
        qs.append(nanws)
        for _ in range(40):                      # rotated quads anywhere on (and around) the face
            th, l1 = rng.uniform(0, np.pi), rng.uniform(0.3, S / 6)
            l2 = l1 * rng.uniform(0.05, 1.0)
            qs.append(W(rng.uniform(-8, S + 8), rng.uniform(-8, S + 8), l1 * np.cos(th), l1 * np.sin(th), l2 * np.sin(th), -l2 * np.cos(th), rng.uniform(0.02, 0.95)))
        lists.append(np.stack(qs[fc:] + qs[:fc]))            # (another order on every face: the cube does not depend on it)
    return lists


@pytest.mark.parametrize("S", [64, 257, 1024])
def test_cube_of_hand_placed_quads_byte_identical(conv, S):
    """Stage B alone (m2s_shadow_from_quads) on quads placed by hand: texel-centre vertices, tile and face borders, zero-area, off-face,
    larger than the face, d >= 1, equal depths, guard band, non-finite — on every face (the atlas rows) and at the x < S / y < S tails."""
    lp = lr.Light(pos=(0.25, -0.5, 0.75))
    lists = hand_lists(S, lp.light_position, lp.far_plane, 100 + S)
    skipped, cube = conv.shadow_from_quads(lists, light_params(lp, (320, 200), S))
    want, wskipped = lr.shadow_cube(lists, S, lp.light_position, lp.far_plane)
    counts = conv.last_shadow_counts()
    print(f"S={S}: hand-placed, skipped {skipped}, texels below 1.0: {(want < 1).mean():.3f}, counts {counts}")
    assert skipped == wskipped == 6 * 4
    assert np.array_equal(cube.view(np.uint32), want.view(np.uint32)), np.argwhere(cube != want)[:8].tolist()
    tiles = (S + lr.sr.TILE - 1) // lr.sr.TILE
    # the cases occur, on the restatement: a quad whose box is the whole face, the corner texels of every face written
    for fc in range(6):
        s = lr.sr.setup(lr.pad24(lists[fc]), S, S)
        boxes = np.concatenate([t["box"][t["valid"]] for t in s["tris"]])
        assert ((boxes[:, 0] == 0) & (boxes[:, 1] == 0) & (boxes[:, 2] == S - 1) & (boxes[:, 3] == S - 1)).any()
        assert (want[fc] <= np.float32(0.9)).all() and (want[fc] < np.float32(0.9)).any()      # the face-sized quad covers every texel
        assert want[fc, S - 1, S - 1] < np.float32(0.21) and want[fc, 0, 0] < np.float32(0.21)   # the corner texels
    assert counts["pairs"] >= 6 * tiles * tiles
    got_lists = [conv.download_shadow_quads(fc, lists[fc].shape[0]) for fc in range(6)]
    assert all(same_bits(g, w) for g, w in zip(got_lists, lists))
    # idempotent; and an empty call afterwards leaves a cube of 1.0
    _, again = conv.shadow_from_quads(lists, light_params(lp, (320, 200), S))
    assert np.array_equal(again.view(np.uint32), cube.view(np.uint32))
    sk0, empty = conv.shadow_from_quads([np.zeros((0, 12), np.float32)] * 6, light_params(lp, (320, 200), S))
    assert sk0 == 0 and (empty == 1.0).all()


# ---- 3. geometry agrees with itself ------------------------------------------------------------------------------------------------
DIRS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 2, 3), (-3, 1, -2), (2, -3, 1), (-1, -2, 0.5), (0.9, 1, 0.1)]


@pytest.mark.parametrize("d", DIRS)
def test_occluder_shadow_lands_where_the_light_ray_meets_the_receiver(conv, d):
    import torch
    W = H = 33
    L = np.float32([0.5, -0.25, 0.75])
    lp = lr.Light(pos=tuple(L), cam=(5, 5, 5))
    d = np.asarray(d, np.float64) / np.linalg.norm(d)
    a = np.cross(d, (0.3, 0.5, 0.8)); a /= np.linalg.norm(a)
    b = np.cross(d, a)
    rec = np.zeros((1, 24), np.float32)
    rec[0, 0:3] = L + d
    # (not isotropic: with c00 == c11 and c01 == 0 the shader's own axis formula is 0 / 0, as in the viewer prepass)
    rec[0, 3] = 1; rec[0, 7] = 1; rec[0, 8:11] = (0.05, 0.04, 0.045); rec[0, 16] = 1
    pp = pp_for(np.eye(4, dtype=np.float32), (W, H), 0, std=1.0, R=1)
    conv.shadow(pp, light_params(lp, (W, H), 256), records=torch.from_numpy(rec).cuda(), download=False)
    u = np.linspace(-1.5, 1.5, W)
    pos = np.zeros((H, W, 4), np.float16)
    pos[..., :3] = L + 3 * d + u[None, :, None] * a + u[:, None, None] * b
    zeros8 = np.zeros((H, W, 4), np.uint8)
    conv.upload_gbuffer([pos, np.zeros((H, W, 4), np.float16), zeros8, None, zeros8])
    frame, counts = conv.relight(light_params(lp, (W, H), 256))
    want = lr.shadow_counts(pos[..., :3].astype(np.float32), conv.download_shadow_cubemap(), lp.light_position, lp.far_plane)
    assert np.array_equal(counts, want)
    assert counts[H // 2, W // 2] == 20
    far_away = (np.abs(u)[None, :] > 1.0) | (np.abs(u)[:, None] > 1.0)
    assert (counts[far_away] == 0).all() and (counts == 20).sum() < W * H // 4


# ---- 4. + 5. relight ---------------------------------------------------------------------------------------------------------------
def check_lit(frame, counts, planes, cube, lp, what):
    want, wcounts, ill = lr.relight(planes, cube, lp)
    assert np.array_equal(counts, wcounts), f"{what}: shadow counts differ at {np.argwhere(counts != wcounts)[:5].tolist()}"
    d = np.abs(frame.astype(np.int32) - want.astype(np.int32))
    share = float(ill.mean())
    dmax = int(d[~ill].max(initial=0))
    print(f"{what}: max |d| on well-conditioned pixels = {dmax} LSB, ill-conditioned share = {share:.5f}")
    assert share <= lr.ILL_SHARE_MAX
    assert (frame[..., 3] == 255).all()
    c64 = lr.shade(planes, wcounts, lp, np.float64)
    nan_px = np.isnan(c64)
    assert (frame[..., :3][nan_px] == 0).all(), f"{what}: NaN pixels must be 0"
    assert dmax <= U8_TOL, (what, dmax)


@pytest.mark.parametrize("case", lr.RELIGHT_CASES)
def test_relight_uploaded_gbuffer_and_cube(conv, case):
    lp = lr.Light()
    W, H, S = case["W"], case["H"], case["S"]
    planes = lr.random_gbuffer(W, H, case["seed"], case["edge"])
    cube = lr.random_cube(S, case["seed"], lp.far_plane)
    conv.upload_gbuffer(planes)
    conv.upload_shadow_cubemap(cube)
    for mode in range(6):                                            # byte copies
        f = conv.relight(light_params(lp, (W, H), S, mode))
        want, _, _ = lr.relight(planes, cube, lp, mode)
        assert np.array_equal(f, want), f"mode {mode}"
    frame, counts = conv.relight(light_params(lp, (W, H), S))
    check_lit(frame, counts, planes, cube, lp, f"uploaded {W}x{H}, S={S}")


def test_render_frame_of_a_small_scene(conv):
    scene = synth.cube_sphere(12, tex_size=32)
    conv.upload_scene(scene)
    conv.convert(64)
    res = (160, 120)
    eye = (1.6, 1.1, 2.3)
    pp = PrepassParams(view_mat=camera.look_at(eye, (0.1, 0.0, -0.1)), proj_mat=camera.perspective(45.0, res[0] / res[1], 0.01, 50.0),
                       renderer_resolution=res, near_plane=0.01, far_plane=50.0, resolution_target=64, render_mode=6)
    lp = lr.Light(pos=(1.0, 2.5, 1.5), cam=eye, intensity=20.0)
    frame, counts = conv.render_frame(pp, light_params(lp, res, 128))
    planes = conv.download_gbuffer()
    cube = conv.download_shadow_cubemap()
    rec = conv.download()
    want_cube, _ = lr.shadow_cube(ref_lists(rec, pp, lp), 128, lp.light_position, lp.far_plane)
    assert np.array_equal(cube.view(np.uint32), want_cube.view(np.uint32))
    assert (cube < 1).any() and counts.max() == 20 and (planes[2][..., 3] > 0).any()
    check_lit(frame, counts, planes, cube, lp, "render_frame")


# ---- 7. error paths ----------------------------------------------------------------------------------------------------------------
def test_errors_and_empty_input(hiplib):
    import torch
    c = Converter(0)
    try:
        lp = lr.Light()
        pp = pp_for(np.eye(4, dtype=np.float32), (16, 8))
        with pytest.raises(_lib.M2SError, match="INVALID"):
            c.relight(light_params(lp, (16, 8), 8))                     # neither G-buffer nor cube
        empty = torch.empty((0, 24), dtype=torch.float32, device="cuda")
        per_face, skipped, cube = c.shadow(pp, light_params(lp, (16, 8), 8), records=empty)
        assert per_face == [0] * 6 and skipped == 0 and cube.shape == (6, 8, 8) and (cube == 1.0).all()
        with pytest.raises(_lib.M2SError, match="INVALID"):
            c.relight(light_params(lp, (16, 8), 8))                     # a cube, but no G-buffer
        from mesh2splat_amd.splat import SplatParams
        c.splat(SplatParams((16, 8), 0), quads=empty, download=False)
        frame, counts = c.relight(light_params(lp, (16, 8), 8))         # lit from an empty G-buffer
        want, wcounts, _ = lr.relight(c.download_gbuffer(), cube, lp)
        assert np.array_equal(counts, wcounts) and np.abs(frame.astype(int) - want.astype(int)).max() <= U8_TOL
        rec = torch.from_numpy(records(10, 1)).cuda()
        for bad in (dict(S=0x1001), dict(mode=7), dict(mode=-1)):
            with pytest.raises(_lib.M2SError, match="INVALID"):
                c.shadow(pp, light_params(lp, (16, 8), bad.get("S", 8), bad.get("mode", 6)), records=rec)
            with pytest.raises(_lib.M2SError, match="INVALID"):
                c.relight(light_params(lp, (16, 8), bad.get("S", 8), bad.get("mode", 6)))
        with pytest.raises(_lib.M2SError, match="INVALID"):
            c.shadow(pp_for(np.eye(4, dtype=np.float32), (0, 8)), light_params(lp, (16, 8), 8), records=rec)
        with pytest.raises(_lib.M2SError, match="INVALID"):
            c.relight(light_params(lp, (8, 16), 8))                     # not the G-buffer's resolution
        from mesh2splat_amd import light as li
        lc = li.to_c(light_params(lp, (16, 8), 8))
        lc.reserved = 1
        import ctypes as C
        assert c._L.m2s_relight(c._h, C.byref(lc)) == 1
        from mesh2splat_amd import prepass as ppm
        pc, _keep = ppm.to_c(pp)
        per = (C.c_uint64 * 6)()
        assert c._L.m2s_shadow(c._h, C.byref(pc), C.byref(lc), rec.data_ptr(), 10, per, None) == 1                 # reserved != 0
        assert c._L.m2s_shadow_from_quads(c._h, C.byref(lc), None, per, None) == 1
        lc.reserved = 0
        assert c._L.m2s_shadow_from_quads(c._h, C.byref(lc), None, per, None) == 0                                 # six empty lists
        per[2] = 3
        assert c._L.m2s_shadow_from_quads(c._h, C.byref(lc), None, per, None) == 1                                 # quads announced, none passed
        for res in ((8193, 8), (16, 8193), (16, -1)):
            with pytest.raises(_lib.M2SError, match="INVALID"):
                c.shadow(pp_for(np.eye(4, dtype=np.float32), res), light_params(lp, (16, 8), 8), records=rec)
        with pytest.raises(_lib.M2SError, match="INVALID"):
            c.shadow(pp_for(np.eye(4, dtype=np.float32), (16, 8), R=0), light_params(lp, (16, 8), 8), records=rec)
        nulls = (C.c_void_p * 5)()
        for W, H in ((0, 8), (8, 0), (8193, 8), (8, 8193)):
            assert c._L.m2s_upload_gbuffer(c._h, nulls, W, H) == 1
        assert c._L.m2s_upload_gbuffer(c._h, None, 8, 8) == 1
        one = np.ones(6, np.float32)
        for S in (0, 4097):
            assert c._L.m2s_upload_shadow_cubemap(c._h, one.ctypes.data, S) == 1
        assert c._L.m2s_upload_shadow_cubemap(c._h, None, 1) == 1
        assert c._L.m2s_upload_shadow_cubemap(c._h, one.ctypes.data, 1) == 0
        frame, counts = c.relight(light_params(lp, (16, 8), 1))             # the G-buffer and a 1-texel cube survive the refused calls
        assert frame.shape == (8, 16, 4)
        with pytest.raises(_lib.M2SError, match="STATE"):
            c.shadow(pp, light_params(lp, (16, 8), 8))                  # no records in the context
    finally:
        c.close()


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------------
def read_png_rgba(path):
    import zlib
    data = open(path, "rb").read()
    pos, idat, W, H = 8, b"", 0, 0
    while pos < len(data):
        ln = int.from_bytes(data[pos:pos + 4], "big")
        typ, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + ln]
        if typ == b"IHDR":
            W, H = int.from_bytes(body[0:4], "big"), int.from_bytes(body[4:8], "big")
        elif typ == b"IDAT":
            idat += body
        pos += 12 + ln
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 4 * W)
    return raw[:, 1:].reshape(H, W, 4)


def test_cli_preview_mode_6_equals_render_frame(tmp_path, hiplib):
    import hashlib
    import os
    import subprocess
    from mesh2splat_amd import gltf_io
    scene = synth.sphere_grid(2, n=5, tex_size=32)
    glb, out = str(tmp_path / "s.glb"), str(tmp_path / "s.ply")
    plain, lit, plain2 = (str(tmp_path / n) for n in ("view.png", "lit.png", "view2.png"))
    gltf_io.write_glb(scene, glb)
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")
    base = [exe, glb, out, "--density", "96", "--preview-size", "320x200"]
    r0 = subprocess.run(base + ["--preview", plain], capture_output=True, text=True)
    r = subprocess.run(base + ["--preview", lit, "--preview-mode", "6"], capture_output=True, text=True)
    r2 = subprocess.run(base + ["--preview", plain2, "--preview-mode", "0", "--light", "1,2,3"], capture_output=True, text=True)
    assert r0.returncode == 0 and r.returncode == 0 and r2.returncode == 0, r.stderr
    # plain --preview: the albedo plane, with or without the new options in their default.  (This shows the new options are inert; that the
    # bytes are the ones the splat pass has always produced is what tests/test_gpu_splat.py::test_cli_preview_png checks, against
    # Converter.splat on the same input — it is unchanged and still passes.)
    assert hashlib.sha256(open(plain, "rb").read()).digest() == hashlib.sha256(open(plain2, "rb").read()).digest()
    assert "preview light:" not in r0.stdout
    img = read_png_rgba(lit)
    H, W = img.shape[:2]
    cam = dict(kv.split("=") for kv in [ln for ln in r.stdout.splitlines() if ln.startswith("preview camera:")][0].split(":", 1)[1].split())
    lig = dict(kv.split("=") for kv in [ln for ln in r.stdout.splitlines() if ln.startswith("preview light:")][0].split(":", 1)[1].split())
    eye, centre = [float(v) for v in cam["eye"].split(",")], [float(v) for v in cam["centre"].split(",")]
    near, far = float(cam["near"]), float(cam["far"])
    lpos, inten = [float(v) for v in lig["position"].split(",")], float(lig["intensity"])
    loaded = gltf_io.load_glb(glb)
    dpos, dint = lr.default_light(np.min([m.bbox_min for m in loaded.meshes], 0), np.max([m.bbox_max for m in loaded.meshes], 0))
    assert np.allclose(lpos, dpos) and np.isclose(inten, dint)
    conv = Converter(0)
    conv.upload_scene(loaded)
    conv.convert(96)
    pp = PrepassParams(view_mat=camera.look_at(eye, centre), proj_mat=camera.perspective(45.0, W / H, near, far),
                       renderer_resolution=(W, H), near_plane=near, far_plane=far, resolution_target=96)
    frame = conv.render_frame(pp, LightParams(tuple(lpos), (1.0, 1.0, 1.0), inten, tuple(eye), near, far, 6, (W, H), 1024, False))
    conv.close()
    assert np.array_equal(img, frame[::-1]), "PNG != relit frame flipped"
    assert (img[..., 3] == 255).all() and img[..., :3].std() > 0
    assert not np.array_equal(img, read_png_rgba(plain))
