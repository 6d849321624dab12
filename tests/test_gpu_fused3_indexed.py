"""-m gpu: the indexed instance of k_fused3 — the strips gather positions, normals and tangents from the upload's table of distinct
vertices (mesh2splat_amd/csrc/m2s_vdedup.hip) through three ids per triangle instead of from the per-corner planes.

Every case converts one scene through the C ABI with set_pipeline("lean") and compares the records byte for byte with the same scene
under set_pipeline("multipass") (which reads the planes), the counter with the oracle's, and asserts through Converter.vertex_table()
which instance ran: the row count against np.unique over the resident corners' 12 attribute words, `in_use` against the rule
(rows < 2^21, rows <= corners / 2).  last_pipeline says "lean" for both instances."""
import numpy as np
import pytest

from mesh2splat_amd import synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.scene import Mesh, Scene

pytestmark = pytest.mark.gpu


def distinct_rows(scene, tri_range=None):
    """-> (distinct vertices, corners) of the resident triangles: all 12 attribute floats compared as bits"""
    words = np.concatenate([np.ascontiguousarray(m.vertices[:, :12], np.float32).view(np.uint32) for m in scene.meshes], axis=0)
    if tri_range:
        words = words[3 * tri_range[0]:3 * (tri_range[0] + tri_range[1])]
    return len(np.unique(words, axis=0)), len(words)


def run(conv, pipeline, scene, R, cap=0, tri_range=None):
    """-> (counter, records as uint32, pipeline that answered, vertex_table())"""
    conv.set_pipeline(pipeline)
    conv.set_triangle_range(*(tri_range if tri_range else (0, None)))
    conv.upload_scene(scene)
    conv.set_max_gaussians(cap)
    total = conv.convert(R)
    return total, conv.download().view(np.uint32).copy(), conv.last_pipeline, conv.vertex_table()


def check(oracle, scene, R, cap=0, tri_range=None, expect="lean", conv=None, use=None):
    """use: whether the table must be in use (None: whatever the rule says for this scene)"""
    first, count = tri_range if tri_range else (0, None)
    ototal = oracle.convert(scene, R, cap=cap, tri_first=first, tri_count=count, count_only=True)[0]
    rows, corners = distinct_rows(scene, tri_range)
    want_use = rows < 2 ** 21 and 2 * rows <= corners
    assert use is None or use == want_use, (rows, corners)
    own = conv is None
    conv = conv or Converter(0)
    try:
        total, rec, ran, vt = run(conv, "lean", scene, R, cap, tri_range)
        with Converter(0) as ref:
            mtotal, mrec, mran, _ = run(ref, "multipass", scene, R, cap, tri_range)
    finally:
        if own:
            conv.close()
    print(f"R={R} cap={cap} range={tri_range}: {total} Gaussians by {ran!r}; {rows} rows of {corners} corners, table {vt}")
    assert mran == "multipass"
    assert expect is None or ran == expect, ran
    assert vt == {"rows": rows, "in_use": want_use}, (vt, rows, corners)
    assert total == ototal and mtotal == ototal, (total, mtotal, ototal)
    assert rec.shape == mrec.shape and rec.shape[0] == (min(ototal, cap) if cap else ototal)
    assert np.array_equal(rec, mrec), "first differing record %d" % int(np.flatnonzero((rec != mrec).any(axis=1))[0])
    return total


def grid_mesh(n, seam_at=None, name="grid", tex_seed=4):
    """n x n quads of the unit square in the plane z = 0 (normal +z, tangent +x), de-indexed; uv = xy, except that the quads right of
    column `seam_at` shift u by 0.5: the vertices of that column then exist with two texture coordinates."""
    tri = []
    for j in range(n):
        for i in range(n):
            du = 0.5 if seam_at is not None and i >= seam_at else 0.0
            q = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
            for a, b, c in ((0, 1, 2), (0, 2, 3)):
                for k in (a, b, c):
                    x, y = q[k][0] / n, q[k][1] / n
                    tri.append((x, y, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, x + du, y))
    return Mesh(name, np.asarray(tri, np.float32), textures=synth.procedural_textures(32, tex_seed),
                bbox_min=np.float32([0, 0, -0.5]), bbox_max=np.float32([1, 1, 0.5]))


def test_small_cube_sphere_through_the_table(hiplib, oracle):
    """6 912 triangles in batches far below 64 (strips across owner waves), at R = 256 — where the ladder may answer instead of
    k_fused3: the bytes are the test there — and at the R of about 10 fragments per triangle, which the indexed instance converts."""
    scene = synth.cube_sphere(24, tex_size=256)
    n256 = check(oracle, scene, 256, expect=None, use=True)
    R10 = int(round(256 * (10.0 * scene.n_triangles / n256) ** 0.5))
    n10 = check(oracle, scene, R10, use=True)
    assert 8.5 * scene.n_triangles < n10 < 11.5 * scene.n_triangles, (R10, n10)


def test_rows_shared_across_meshes(hiplib, oracle):
    """Two meshes with the same vertices: the second mesh's triangles use the rows of the first; the mesh boundary lies inside a batch."""
    scene = synth.colocated_spheres(2, 24, 64)
    rows, corners = distinct_rows(scene)
    one, _ = distinct_rows(Scene([scene.meshes[0]]))
    assert rows == one and corners == 2 * 3 * scene.meshes[0].n_triangles
    check(oracle, scene, 150, use=True)


@pytest.mark.parametrize("over", [False, True])
def test_shared_mesh_and_soup_on_both_sides_of_the_sharing_threshold(hiplib, oracle, over):
    """A cube-sphere (shared vertices, combo texture) and a soup without maps (every corner its own row) in one scene: with N soup
    triangles rows = U + 3 N against corners = C + 3 N; N is the largest with 2 rows <= corners, or one more."""
    sphere = synth.cube_sphere(24, tex_size=64).meshes[0]
    U, Cn = distinct_rows(Scene([sphere]))
    N = (Cn - 2 * U) // 3 + (1 if over else 0)
    soup = synth.random_soup(N, seed=6, tri_size=0.08).meshes[0]
    sphere.bbox_min = sphere.bbox_max = soup.bbox_min = soup.bbox_max = None
    soup.name = "soup_1"
    scene = Scene([sphere, soup])
    rows, corners = distinct_rows(scene)
    assert rows == U + 3 * N and corners == Cn + 3 * N and (2 * rows > corners) == over
    check(oracle, scene, 160, use=not over)


def test_uv_seam_makes_two_rows_of_one_position(hiplib, oracle):
    scene = Scene([grid_mesh(12, seam_at=6)])
    rows, corners = distinct_rows(scene)
    assert rows == 13 * 13 + 13 and corners == 12 * 12 * 6
    assert distinct_rows(Scene([grid_mesh(12)]))[0] == 13 * 13
    check(oracle, scene, 96, use=True)


def test_triangle_range_uses_the_ids_of_its_shard(hiplib, oracle):
    scene = synth.cube_sphere(24, tex_size=64)
    check(oracle, scene, 160, tri_range=(101, 2999), use=True)


def test_cap_inside_a_strip_and_a_deferred_triangle_inside_a_shared_mesh(hiplib, oracle):
    """One triangle of a grid grown beyond the 8 x 8 box (deferred to k_emit_big, which reads the planes; its workgroup's strips take
    the irregular path), then a cap that ends the output in the middle of a strip behind it."""
    m = grid_mesh(20)
    v = m.vertices.reshape(-1, 3, 12).copy()
    v[301, :, 0:3] = np.float32([[0.2, 0.2, 0.0], [0.7, 0.25, 0.0], [0.3, 0.75, 0.0]])
    scene = Scene([Mesh("big", v.reshape(-1, 12), textures=m.textures, bbox_min=m.bbox_min, bbox_max=m.bbox_max)])
    R = 128
    cnt = oracle.count_per_triangle(scene, R).astype(np.int64)
    assert cnt[301] > 500 and cnt.sum() - cnt[301] > 500
    full = check(oracle, scene, R, use=True)
    assert full == cnt.sum()
    cap = int(cnt[:500].sum()) + 29
    assert cnt[:302].sum() + 64 < cap < full - 64 and cap % 64
    check(oracle, scene, R, cap=cap, use=True)


def test_second_scene_in_the_same_context_gets_its_own_table(hiplib, oracle):
    """No stale table: a sphere, then a grid with a seam, then a soup that takes no table at all, then the sphere again."""
    sphere = synth.cube_sphere(24, tex_size=64)
    grid = Scene([grid_mesh(12, seam_at=5, tex_seed=8)])
    soup = synth.random_soup(300, seed=21, tri_size=0.1, textures=synth.procedural_textures(16, 2))
    with Converter(0) as conv:
        check(oracle, sphere, 150, conv=conv, use=True)
        check(oracle, grid, 96, conv=conv, use=True)
        check(oracle, soup, 128, conv=conv, use=False)
        check(oracle, sphere, 150, conv=conv, use=True)
