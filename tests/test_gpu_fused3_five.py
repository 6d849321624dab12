"""-m gpu: seams of k_fused3's LDS protocol — irregular workgroups (a deferred triangle in the last or the first wave, next to a
regular workgroup), texture coordinates at seams and outside [0, 1), meshes with and without maps in one batch, a full entry stream —
on both instances of the kernel.  (The name is from the five-workgroup layout of DESIGN 6.3, whose seams these are.)

Every case converts one scene through the C ABI with set_pipeline("lean") and compares the records byte for byte with the same scene
under set_pipeline("multipass"), the counter with the oracle's, and asserts which instance ran (Converter.vertex_table()).  Cases
stated for a soup (every corner its own vertex: the plane instance) run a second time on a soup of fans, whose shared vertices put
it through the indexed instance.

Small scenes run in work-balanced batches of 8 .. 64 triangles per wave (run_pass builds the table from the exact counts at the R
the upload prepared for); batch_table() restates that rule, so that a case can say which wave of which workgroup holds a triangle.
"""
import numpy as np
import pytest

from mesh2splat_amd import synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.scene import Mesh, Scene

from test_gpu_fused3_entries import UNIT_BOX, flat_triangles, right_triangles
from test_gpu_fused3_indexed import check as check_table
from test_gpu_fused3_indexed import distinct_rows

pytestmark = pytest.mark.gpu

ENTRIES = 4096              # k_fused3's entry stream per workgroup (both instances), and k_fused2's


def check5(oracle, scene, R, use, cap=0, expect="lean"):
    """lean against multipass byte for byte, counter against the oracle, and which instance ran"""
    with Converter(0) as conv:
        conv.set_resolution_hint(R)
        return check_table(oracle, scene, R, cap=cap, expect=expect, conv=conv, use=use)


# ---- which wave holds which triangle ----------------------------------------------------------------------------------------------

def batch_table(cnt):
    """first triangle of every batch (and the triangle count behind the last): the work-balanced table of a scene too small for
    64-triangle batches (m2s_pass.cpp: 214 per triangle + 140 per fragment, batches close at multiples of 8)"""
    n = len(cnt)
    per = (n + 3071) // 3072
    tpw = min(max((per + 7) & ~7, 8), 64)
    assert tpw < 64
    work = 214.0 + 140.0 * np.asarray(cnt, np.float64)
    quota = work.sum() / ((n + tpw - 1) // tpw)
    first, acc, in_batch = [0], 0.0, 0
    for g in range(0, n, 8):
        ge = min(g + 8, n)
        gc = float(work[g:ge].sum())
        if in_batch and (in_batch + (ge - g) > 64 or acc + 0.5 * gc >= quota * len(first)):
            first.append(g)
            in_batch = 0
        acc += gc
        in_batch += ge - g
    first.append(n)
    return np.asarray(first)


def workgroup_of(cnt, t):
    """-> (wave of triangle t inside its workgroup, [(first, end) of the workgroup's four batches])"""
    first = batch_table(cnt)
    b = int(np.searchsorted(first, t, side="right")) - 1
    b0 = b & ~3
    return b - b0, [(int(first[k]), int(first[k + 1])) for k in range(b0, min(b0 + 4, len(first) - 1))]


# ---- scenes -----------------------------------------------------------------------------------------------------------------------

BIG = np.float32([[0.2, 0.2, 0.5], [0.7, 0.25, 0.5], [0.3, 0.75, 0.55]])    # > 500 fragments at R = 128: deferred to k_emit_big


def fan_soup(n_fans, seed, tri_size, textures):
    """A soup of closed fans of six triangles: 7 distinct vertices for 18 corners, so the upload keeps a vertex table; positions,
    normals, tangents and texture coordinates (-0.5 .. 2.5: REPEAT on both sides of [0, 1)) random per VERTEX."""
    rng = np.random.default_rng(seed)
    tris = []
    for _ in range(n_fans):
        c = rng.uniform(0.05, 0.95, 3)
        size = tri_size * rng.uniform(0.15, 1.0) ** 2
        e1, e2 = rng.normal(size=(2, 3))
        e1 /= np.linalg.norm(e1)
        e2 -= e1 * (e1 @ e2)
        e2 /= np.linalg.norm(e2)
        ang = np.arange(6) * (np.pi / 3) + rng.uniform(0, 1)
        rad = size * rng.uniform(0.6, 1.0, 6)
        pos = np.concatenate([c[None], c + (np.cos(ang) * rad)[:, None] * e1 + (np.sin(ang) * rad)[:, None] * e2], axis=0)
        att = np.zeros((7, 12), np.float32)
        att[:, 0:3] = pos
        nrm = rng.normal(size=(7, 3))
        tng = rng.normal(size=(7, 3))
        att[:, 3:6] = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
        att[:, 6:9] = tng / np.linalg.norm(tng, axis=-1, keepdims=True)
        att[:, 9] = rng.choice([-1.0, 1.0], 7)
        att[:, 10:12] = rng.uniform(-0.5, 2.5, (7, 2))
        for k in range(6):
            tris.append(att[[0, 1 + k, 1 + (k + 1) % 6]])
    return np.asarray(tris, np.float32)            # (6 n_fans, 3, 12)


def soup_vertices(kind, n_tri, seed, tri_size=0.1):
    tex = synth.procedural_textures(16, 2)
    if kind == "soup":
        s = synth.random_soup(n_tri, seed=seed, tri_size=tri_size, textures=tex)
        return s.meshes[0].vertices.reshape(n_tri, 3, -1).copy(), tex
    return fan_soup(n_tri // 6, seed, tri_size, tex), tex


def with_big(v, at):
    v = v.copy()
    v[at, :, 0:3] = BIG
    return v


def scene_of(v, tex, name="big"):
    return Scene([Mesh(name, v.reshape(-1, v.shape[2]), base_color=(0.8, 0.6, 0.4, 0.9), textures=tex)])


def place_big(oracle, v, tex, R, near, want_wave):
    """The soup with BIG at the index closest to `near` whose batch is wave `want_wave` of a workgroup of four batches that all hold
    covered small triangles.  -> (scene, index, counts)"""
    for at in sorted(range(max(near - 24, 0), min(near + 24, len(v))), key=lambda i: abs(i - near)):
        scene = scene_of(with_big(v, at), tex)
        cnt = oracle.count_per_triangle(scene, R).astype(np.int64)
        wave, batches = workgroup_of(cnt, at)
        small = cnt.copy()
        small[at] = 0
        if wave == want_wave and len(batches) == 4 and all(small[a:b].any() for a, b in batches) and cnt[at] > 500:
            return scene, at, cnt
    raise AssertionError("no index near %d puts the deferred triangle into wave %d" % (near, want_wave))


# ---- deferred triangles: the irregular path ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["soup", "fans"])
@pytest.mark.parametrize("near, wave", [(290, 3), (5, 0)])
def test_deferred_triangle_in_the_last_and_in_the_first_wave(hiplib, oracle, kind, near, wave):
    """An irregular workgroup: one triangle of more than 500 fragments (deferred), in the workgroup's last wave — the earlier waves
    stored their tskip before that wave raised the flag — and in its first; every wave of the workgroup has covered small triangles,
    whose records go through tskip.  Then a cap that ends inside a strip behind the deferred triangle."""
    R = 128
    v, tex = soup_vertices(kind, 300, 21)
    scene, at, cnt = place_big(oracle, v, tex, R, near, wave)
    print(f"{kind}: deferred triangle {at} ({cnt[at]} fragments), wave {wave} of {workgroup_of(cnt, at)[1]}")
    use = kind == "fans"
    full = check5(oracle, scene, R, use)
    assert full == cnt.sum() and cnt.sum() - cnt[at] > 500
    pre = int(cnt[:at + 1].sum())
    rest = int(full) - pre
    assert rest >= 3, rest
    cap = pre + min(rest // 2, 5 * 64 + 29)
    if cap % 64 == 0:
        cap += 1
    assert pre < cap < full, (pre, cap, full)
    check5(oracle, scene, R, use, cap=cap)


@pytest.mark.parametrize("kind", ["soup", "fans"])
def test_regular_and_irregular_workgroups_in_one_launch(hiplib, oracle, kind):
    """Two soups in one mesh, the deferred triangle only in the second: regular workgroups (records staged in LDS) and an irregular
    one (records stored per lane through tskip) side by side in the same launch.  (Both halves of triangles small enough that
    none but the one is deferred: whatever the projection axis, a triangle's extent stays under 7 pixels — an 8 x 8 box at most.)"""
    R = 128
    v, tex = soup_vertices(kind, 300, 21, tri_size=0.02)
    v2, _ = soup_vertices(kind, 300, 22, tri_size=0.02)
    both = np.concatenate([v, v2], axis=0)
    pos = both[..., 0:3].astype(np.float64)
    assert ((pos.max(axis=1) - pos.min(axis=1)).max() / (pos.max(axis=(0, 1)) - pos.min(axis=(0, 1))).min()) * R < 7.0
    both = with_big(both, 300 + 286)
    scene = scene_of(both, tex)
    cnt = oracle.count_per_triangle(scene, R).astype(np.int64)
    first = batch_table(cnt)
    at = 300 + 286
    b = int(np.searchsorted(first, at, side="right")) - 1
    assert cnt[at] > 500 and cnt[:300].sum() > 100
    regular = [(int(first[k]), int(first[k + 4])) for k in range(0, (b & ~3), 4)]
    assert len(regular) >= 4 and all(cnt[a:e].sum() > 0 for a, e in regular[-2:])      # the neighbours in front of it have records to stage
    assert check5(oracle, scene, R, kind == "fans") == cnt.sum()


# ---- texture coordinates at seams and wraps ----------------------------------------------------------------------------------------

def uv_grid(n, name, textures, seam_at=None, su=1.0, ou=0.0, sv=1.0, ov=0.0, color=(1.0, 1.0, 1.0, 1.0)):
    """n x n quads of the unit square (z = 0, normal +z, tangent +x), de-indexed; uv = (su x + ou, sv y + ov), and the quads right of
    column `seam_at` shift u by 0.5: that column's vertices exist with one position and two coordinates, inside one quad row's pairs."""
    tri = []
    for j in range(n):
        for i in range(n):
            du = 0.5 if seam_at is not None and i >= seam_at else 0.0
            q = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
            for a, b, c in ((0, 1, 2), (0, 2, 3)):
                for k in (a, b, c):
                    x, y = q[k][0] / n, q[k][1] / n
                    tri.append((x, y, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, su * x + ou + du, sv * y + ov))
    return Mesh(name, np.asarray(tri, np.float32), base_color=color, textures=textures, **UNIT_BOX)


def test_uv_seam_one_position_two_coordinates(hiplib, oracle):
    """The seam column's vertices are two rows each (same position, normal, tangent; u and u + 0.5): a strip must shade with the coordinates
    of the triangle's own corner, on both sides of the seam, whichever row supplied the position."""
    scene = Scene([uv_grid(20, "seam", synth.procedural_textures(64, 4), seam_at=9)])      # quads of 8 x 8 pixels at R = 160
    rows, corners = distinct_rows(scene)
    assert rows == 21 * 21 + 21 and corners == 20 * 20 * 6
    check5(oracle, scene, 160, True)


def test_coordinates_outside_the_unit_square_and_negative(hiplib, oracle):
    """u from -0.75 to 2.25 with a seam on top, v from -0.25 down to -1.75: REPEAT wraps both ways, and the interpolation runs on the
    unwrapped values."""
    m = uv_grid(18, "wrap", synth.procedural_textures(64, 5), seam_at=7, su=3.0, ou=-0.75, sv=-1.5, ov=-0.25)    # 8 x 8 pixels at R = 144
    uv = m.vertices[:, 10:12]
    assert uv[:, 0].min() < 0 and uv[:, 0].max() > 2 and uv[:, 1].max() < 0 and uv[:, 1].min() < -1
    check5(oracle, Scene([m]), 144, True)


def test_mesh_without_maps_shares_a_batch_with_one_that_has_them(hiplib, oracle):
    """98 triangles with maps, then 98 without: batches start at multiples of 8, so triangles 96 .. 103 are one batch's and strips
    hold fragments of both meshes; the second mesh samples nothing."""
    a = uv_grid(7, "mapped", synth.procedural_textures(64, 6), su=2.0, ou=-0.5)
    b = uv_grid(7, "plain", {}, color=(0.3, 0.9, 0.5, 1.0))
    a.bbox_min = a.bbox_max = b.bbox_min = b.bbox_max = None
    b.vertices[:, 2] = 0.25                                  # (its own plane: no rows shared with the first mesh)
    scene = Scene([a, b])
    R = 56                                                  # quads of 8 x 8 pixels
    cnt = oracle.count_per_triangle(scene, R)
    assert a.vertices.shape[0] // 3 == 98 and cnt[96:98].sum() > 0 and cnt[98:104].sum() > 0
    check5(oracle, scene, R, True)


# ---- the entry stream's capacity, from both sides ---------------------------------------------------------------------------------

def capacity_scene(R, legs_px, seam=False):
    """174 080 triangles of one fragment each on a grid of two pixels' pitch — enough for 64-triangle batches: a workgroup is 256
    consecutive triangles — as pairs that share their hypotenuse's vertices (a vertex table), except workgroup 300: 256 right triangles
    with legs of `legs_px` pixels."""
    px = 1.0 / R
    n = 680 * 256
    idx = np.arange(n)
    tris = right_triangles(np.stack([(2 * (idx % 512) + 0.1) * px, (2 * (idx // 512) + 0.1) * px], axis=1), 1.5 * px)
    k = np.arange(256)
    tris[256 * 300:256 * 301] = right_triangles(np.stack([(9 * (k % 100) + 0.55) * px, (700 + 9 * (k // 100) + 0.55) * px], axis=1), legs_px * px)
    return Scene([Mesh("capacity", flat_triangles(tris), textures=synth.procedural_textures(64, 7), **UNIT_BOX)])


def shared_capacity_scene(R, legs_px):
    """The same with every triangle twice (the second copy behind the first, in the same mesh): two corners per row, so the scene runs
    the indexed instance; workgroups 300 and 980 hold the larger triangles."""
    s = capacity_scene(R, legs_px)
    m = s.meshes[0]
    return Scene([Mesh("capacity2", np.concatenate([m.vertices, m.vertices], axis=0), textures=m.textures, **UNIT_BOX)])


@pytest.mark.parametrize("frags, legs", [(10, 5.4), (15, 6.4)])
def test_indexed_instance_capacity_from_below(hiplib, oracle, frags, legs):
    """256 x 10 = 2 560 and 256 x 15 = 3 840 entries in one workgroup of the indexed instance: both fit the stream and run lean.  (The
    other side, 256 x 21 = 5 376, is test_gpu_fused3_entries.py's overflow case.)"""
    assert 256 * frags <= ENTRIES
    R = 1024
    scene = shared_capacity_scene(R, legs)
    cnt = oracle.count_per_triangle(scene, R)
    n = 680 * 256
    for w in (300, 300 + 680):
        assert np.all(cnt[256 * w:256 * (w + 1)] == frags)
    assert cnt.sum() == 2 * (n - 256) + 2 * 256 * frags and np.count_nonzero(cnt != 1) == 512
    check5(oracle, scene, R, True)


def test_plane_instance_keeps_its_capacity(hiplib, oracle):
    """The same 3 840 entries in a scene without a vertex table (every corner its own row): the plane instance runs lean as well."""
    R = 1024
    scene = capacity_scene(R, 6.4)
    cnt = oracle.count_per_triangle(scene, R)
    sel = np.arange(256 * 300, 256 * 301)
    assert np.all(cnt[sel] == 15) and np.all(np.delete(cnt, sel) == 1)
    check5(oracle, scene, R, False)
