"""-m gpu: the geometry planes — Quaternion, Scale and the box-normalised orthogonal UVs of every resident triangle, computed once per
upload (mesh2splat_amd/csrc/m2s_geoplanes.hip) and read by k_fused3's triangle phase in place of the positions (the kGeo instances).

The method is tests/test_gpu_fused3_indexed.py's: every `check` converts one scene at one R and cap with set_pipeline("lean") and
compares the records byte for byte with set_pipeline("multipass") on a second context (which computes its geometry itself), the counter
with the oracle's, and Converter.geo_planes() with the rule: planes are built, and in use, exactly when the scene can take the lean form
(every mesh samples three equally sized maps or none) and has between 1 and 2^22 resident triangles.  A stale or wrong plane word shows
up as a differing record."""
import numpy as np
import pytest

from mesh2splat_amd import synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.scene import Mesh, Scene
from test_gpu_fused3_indexed import distinct_rows, grid_mesh

pytestmark = pytest.mark.gpu


def lean_ok(scene):
    """every mesh has its three maps in one size (the interleaved texture) or no map at all"""
    for m in scene.meshes:
        shapes = {t.shape[:2] for t in m.textures.values()}
        if m.textures and (len(m.textures) != 3 or len(shapes) != 1):
            return False
    return True


def planes_rule(scene, tri_range=None):
    n = tri_range[1] if tri_range else scene.n_triangles
    use = lean_ok(scene) and 1 <= n <= 2 ** 22
    return {"bytes": 48 * n if use else 0, "in_use": use}


def upload(conv, pipeline, scene, tri_range=None, hint=None):
    conv.set_pipeline(pipeline)
    conv.set_triangle_range(*(tri_range if tri_range else (0, None)))
    if hint is not None:
        conv.set_resolution_hint(hint)
    conv.upload_scene(scene)


def check(oracle, scene, R, cap=0, tri_range=None, expect="lean", conv=None, uploaded=False, table=None, hint=None):
    """conv: the lean context (None: one of its own); uploaded: it holds the scene already (no upload here);
    table: whether the vertex table must be in use (None: not asserted)"""
    first, count = tri_range if tri_range else (0, None)
    ototal = oracle.convert(scene, R, cap=cap, tri_first=first, tri_count=count, count_only=True)[0]
    own = conv is None
    conv = conv or Converter(0)
    try:
        if not uploaded:
            upload(conv, "lean", scene, tri_range, hint)
        conv.set_max_gaussians(cap)
        total = conv.convert(R)
        rec, ran, gp, vt = conv.download().view(np.uint32).copy(), conv.last_pipeline, conv.geo_planes(), conv.vertex_table()
        with Converter(0) as ref:
            upload(ref, "multipass", scene, tri_range)
            ref.set_max_gaussians(cap)
            mtotal = ref.convert(R)
            mrec, mran = ref.download().view(np.uint32).copy(), ref.last_pipeline
    finally:
        if own:
            conv.close()
    print(f"R={R} cap={cap} range={tri_range}: {total} Gaussians by {ran!r}; planes {gp}, table {vt}")
    assert mran == "multipass"
    assert expect is None or ran == expect, ran
    assert gp == planes_rule(scene, tri_range), (gp, planes_rule(scene, tri_range))
    assert table is None or vt["in_use"] == table, vt
    assert total == ototal and mtotal == ototal, (total, mtotal, ototal)
    assert rec.shape == mrec.shape and rec.shape[0] == (min(ototal, cap) if cap else ototal)
    assert np.array_equal(rec, mrec), "first differing record %d" % int(np.flatnonzero((rec != mrec).any(axis=1))[0])
    return total


def test_one_upload_serves_every_resolution(hiplib, oracle):
    """The planes do not depend on R: one upload, prepared for an R that is never converted at, then three conversions."""
    scene = synth.cube_sphere(24, tex_size=64)
    assert scene.n_triangles == 6912
    n96 = oracle.convert(scene, 96, count_only=True)[0]
    R10 = int(round(96 * (10.0 * scene.n_triangles / n96) ** 0.5))
    assert R10 not in (64, 96, 150)
    with Converter(0) as conv:
        upload(conv, "lean", scene, hint=64)
        assert conv.geo_planes() == {"bytes": 48 * 6912, "in_use": True}
        for R in (96, 150, R10):
            n = check(oracle, scene, R, conv=conv, uploaded=True, table=True)
        assert 8.5 * scene.n_triangles < n < 11.5 * scene.n_triangles, (R10, n)


def hostile_grid(scale=1.0):
    """The 12 x 12 grid with (a) vertices exactly on the planes of the box (x = 0, y = 0: the grid has them; one more is moved onto z = -0.5),
    (b) a triangle with an edge of length zero and one whose corners lie on a line; the whole mesh, positions and box, times `scale`."""
    m = grid_mesh(12)
    v = m.vertices.reshape(-1, 3, 12).copy()
    assert (v[0, 0, 0:2] == 0).all()                       # (a) rel = 0 in both axes of the projection
    v[40, 1, 2] = -0.5                                     # (a) ... and a corner on the box's lower z plane (tilts the triangle)
    v[77, 1, 0:3] = v[77, 0, 0:3]                          # (b) zero-length edge
    v[130, :, 0:3] = np.float32([[0.25, 0.25, 0.0], [0.5, 0.5, 0.0], [0.75, 0.75, 0.0]])   # (b) zero area, three distinct corners
    v[..., 0:3] *= np.float32(scale)
    return Scene([Mesh("hostile", v.reshape(-1, 12), textures=m.textures, bbox_min=m.bbox_min * np.float32(scale),
                       bbox_max=m.bbox_max * np.float32(scale))])


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -45], ids=["unit", "2^-45"])
def test_operands_outside_the_fast_ranges(hiplib, oracle, scale):
    """geo_setup takes its IEEE forms for a whole wave when one operand leaves the proven range of the short forms: a difference of
    exactly zero, a zero length, lengths of 2^-49.  The plane kernel's waves are not k_fused3's batches; the bits must not depend on it."""
    scene = hostile_grid(scale)
    cnt = oracle.count_per_triangle(scene, 96)
    assert cnt[77] == 0 and cnt[130] == 0 and cnt.sum() > 2000
    check(oracle, scene, 96)


def test_two_meshes_in_one_batch(hiplib, oracle):
    """Two meshes whose boundary lies inside a wave of the plane kernel and inside a batch of k_fused3, each with its own box: the
    second sphere is larger, so the cumulative box grows with it.  (synth.colocated_spheres(2, 24, 64) has 6 912 = 108 x 64 triangles
    per mesh — its boundary falls on a batch boundary; it is converted as well, for the two meshes' shared box.)"""
    a = synth.cube_sphere(23, tex_size=64).meshes[0]
    b = synth.cube_sphere(23, tex_size=64, name="sphere_1").meshes[0]
    vb = b.vertices.copy()
    vb[:, 0:3] *= np.float32(1.5)
    scene = Scene([Mesh("sphere_0", a.vertices, textures=a.textures), Mesh("sphere_1", vb, textures=b.textures)])
    assert scene.meshes[0].n_triangles % 64 != 0 and scene.meshes[0].n_triangles % 8 != 0
    assert not np.array_equal(scene.meshes[0].bbox_max, scene.meshes[1].bbox_max)
    check(oracle, scene, 150)
    check(oracle, synth.colocated_spheres(2, 24, 64), 150, table=True)


def test_shard_has_planes_of_its_own_triangles(hiplib, oracle):
    check(oracle, synth.cube_sphere(24, tex_size=64), 160, tri_range=(101, 2999), table=True)


def test_deferred_triangle_and_a_cap_inside_a_strip(hiplib, oracle):
    """One triangle of a grid grown beyond the 8 x 8 box: its wave takes the full raster setup from the planes' ou / ov and defers it to
    k_emit_big; then a cap that ends the output in the middle of a strip behind it."""
    m = grid_mesh(20)
    v = m.vertices.reshape(-1, 3, 12).copy()
    v[301, :, 0:3] = np.float32([[0.2, 0.2, 0.0], [0.7, 0.25, 0.0], [0.3, 0.75, 0.0]])
    scene = Scene([Mesh("big", v.reshape(-1, 12), textures=m.textures, bbox_min=m.bbox_min, bbox_max=m.bbox_max)])
    R = 128
    cnt = oracle.count_per_triangle(scene, R).astype(np.int64)
    assert cnt[301] > 500 and cnt.sum() - cnt[301] > 500
    full = check(oracle, scene, R)
    assert full == cnt.sum()
    cap = int(cnt[:500].sum()) + 29
    assert cnt[:302].sum() + 64 < cap < full - 64 and cap % 64
    check(oracle, scene, R, cap=cap)


def test_no_stale_planes_in_a_context(hiplib, oracle):
    """A sphere, a smaller grid, a soup with one map only (no lean form: no planes), then the sphere again."""
    sphere = synth.cube_sphere(24, tex_size=64)
    grid = Scene([grid_mesh(12, seam_at=5, tex_seed=8)])
    one_map = {"baseColorTexture": synth.procedural_textures(16, 2)["baseColorTexture"]}
    soup = synth.random_soup(300, seed=21, tri_size=0.1, textures=one_map)
    assert lean_ok(sphere) and lean_ok(grid) and not lean_ok(soup)
    with Converter(0) as conv:
        check(oracle, sphere, 150, conv=conv)
        check(oracle, grid, 96, conv=conv)
        check(oracle, soup, 128, conv=conv, expect=None)
        assert conv.geo_planes() == {"bytes": 0, "in_use": False}
        check(oracle, sphere, 150, conv=conv)


def test_soup_without_a_vertex_table_runs_the_plane_instance(hiplib, oracle):
    """Every corner of a soup is its own vertex: no table, k_fused3<false, true> — geometry planes with the per-corner attribute planes."""
    soup = synth.random_soup(300, seed=21, tri_size=0.1, textures=synth.procedural_textures(16, 2))
    rows, corners = distinct_rows(soup)
    assert 2 * rows > corners
    check(oracle, soup, 128, table=False)
