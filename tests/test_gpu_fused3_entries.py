"""-m gpu: k_fused3's one-byte entry stream (bit of the mask | first << 6), decoded through the per-wave prefix sums `cum`.

Every case converts one scene through the C ABI with set_pipeline("lean") and compares the records byte for byte with the same
scene under set_pipeline("multipass"), and the counter with the oracle's.  The decode can go wrong where a strip of 64 entries
meets something other than "the next fragment of the same wave": the cases are those seams.

Scenes of fewer than ~172 k triangles run in batches of 8 .. 64 triangles per wave (work-balanced batch table), so a 64-entry strip
of a small scene crosses owner waves all the time; the overflow case needs 64-triangle batches and is the one larger scene.
"""
import numpy as np
import pytest

from mesh2splat_amd import synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.scene import Mesh, Scene

pytestmark = pytest.mark.gpu


def run(pipeline, scene, R, cap=0, tri_range=None):
    """-> (counter, records as uint32, pipeline that answered)"""
    with Converter(0) as c:
        c.set_pipeline(pipeline)
        if tri_range:
            c.set_triangle_range(*tri_range)
        c.upload_scene(scene)
        c.set_max_gaussians(cap)
        total = c.convert(R)
        rec = c.download().view(np.uint32).copy()
        return total, rec, c.last_pipeline


def check(oracle, scene, R, cap=0, tri_range=None, expect="lean"):
    first, count = tri_range if tri_range else (0, None)
    ototal = oracle.convert(scene, R, cap=cap, tri_first=first, tri_count=count, count_only=True)[0]
    total, rec, ran = run("lean", scene, R, cap, tri_range)
    mtotal, mrec, mran = run("multipass", scene, R, cap, tri_range)
    print(f"R={R} cap={cap} range={tri_range}: {total} Gaussians, lean setting answered by {ran!r}")
    assert mran == "multipass"
    assert expect is None or ran == expect, ran
    assert total == ototal and mtotal == ototal, (total, mtotal, ototal)
    assert rec.shape == mrec.shape and rec.shape[0] == (min(ototal, cap) if cap else ototal)
    assert np.array_equal(rec, mrec), "first differing record %d" % int(np.flatnonzero((rec != mrec).any(axis=1))[0])
    return total


def flat_triangles(corners, stride=12):
    """(T, 3, 2) corner positions in the unit square of the plane z = 0 -> de-indexed vertices (normal +z, tangent +x, uv = xy)"""
    corners = np.asarray(corners, np.float32)
    v = np.zeros((corners.shape[0], 3, stride), np.float32)
    v[..., 0:2] = corners
    v[..., 5] = 1.0
    v[..., 6] = 1.0
    v[..., 9] = 1.0
    v[..., 10:12] = corners
    return v.reshape(-1, stride)


UNIT_BOX = dict(bbox_min=np.float32([0, 0, -0.5]), bbox_max=np.float32([1, 1, 0.5]))


def right_triangles(origins, leg):
    o = np.asarray(origins, np.float64)
    return np.stack([o, o + [leg, 0.0], o + [0.0, leg]], axis=1)


def alternating_soup():
    """600 triangles; every second one has its three corners in one point, the others are the sizes a soup comes in (many sub-pixel)"""
    s = synth.random_soup(600, seed=11, tri_size=0.05, textures=synth.procedural_textures(16, 3))
    v = s.meshes[0].vertices.reshape(600, 3, -1).copy()
    v[1::2, :, 0:3] = v[1::2, 0:1, 0:3]
    return Scene([Mesh("alt", v.reshape(-1, v.shape[2]), base_color=(0.8, 0.6, 0.4, 0.9), textures=s.meshes[0].textures)])


def largest_small_triangle_scene(R):
    """Triangles of one fragment each (legs of 1.5 pixels around a pixel centre) and, between them, the largest triangle a workgroup
    shades itself: legs of 8.4 pixels (the limit is an extent of 9) over an 8 x 8 box of pixel centres, 28 of them covered."""
    px = 1.0 / R
    cells = [(x, y) for y in range(2, R - 2, 3) for x in range(2, R - 12, 3)][:200]
    tris = right_triangles([((x + 0.1) * px, (y + 0.1) * px) for x, y in cells], 1.5 * px)
    big = right_triangles([((R - 10 + 0.55) * px, (4 + 0.55) * px)], 8.4 * px)
    tris = np.concatenate([tris[:101], big, tris[101:]], axis=0)
    return Scene([Mesh("mask", flat_triangles(tris), textures=synth.procedural_textures(32, 5), **UNIT_BOX)])


def test_small_cube_sphere_strips_across_owner_waves(hiplib, oracle):
    """n = 24 (6 912 triangles, batches far below 64 triangles: a strip holds entries of two, three and more waves; the last strip of
    most workgroups is short), at R = 256 and at the R with about 10 fragments per triangle.  (At R = 256 the scene has 24.7 fragments
    per triangle: its work-balanced batches may hold more than the stream's 4096 entries per workgroup, and then the ladder answers;
    which form does is not this test's business at that R, the bytes are.)"""
    scene = synth.cube_sphere(24, tex_size=256)
    n256 = check(oracle, scene, 256, expect=None)
    R10 = int(round(256 * (10.0 * scene.n_triangles / n256) ** 0.5))
    n10 = check(oracle, scene, R10)
    assert 8.5 * scene.n_triangles < n10 < 11.5 * scene.n_triangles, (R10, n10)


def test_alternating_covered_and_empty_triangles(hiplib, oracle):
    """Every second triangle has no fragment: equal prefix sums repeat, slots and lanes differ; many covered triangles have exactly
    one fragment (an entry that is nothing but its `first` flag)."""
    scene = alternating_soup()
    R = 96
    cnt = oracle.count_per_triangle(scene, R)
    assert not cnt[1::2].any() and (cnt[0::2] == 1).sum() > 20 and (cnt[0::2] > 1).sum() > 20 and (cnt[0::2] == 0).sum() > 20
    check(oracle, scene, R)


def test_largest_mask_next_to_single_fragments(hiplib, oracle):
    """The densest mask the kernel meets — no triangle covers all 64 centres of its 8 x 8 box: one of at most nine pixels' extent
    covers less than half of them; a right triangle with legs of 8.4 pixels covers 28 — between triangles of one fragment each: one
    triangle's entries are close to half a strip, its neighbours' one entry each."""
    R = 64
    scene = largest_small_triangle_scene(R)
    cnt = oracle.count_per_triangle(scene, R)
    assert cnt[101] == 28 and np.all(np.delete(cnt, 101) == 1), (cnt[101], np.unique(np.delete(cnt, 101)))
    check(oracle, scene, R)


def test_two_materials_in_one_batch_one_without_maps(hiplib, oracle):
    """The mesh boundary lies inside a batch (100 is no multiple of 8, let alone 64): strips that hold fragments of both meshes take
    two turns of the mesh loop; the second mesh has no maps."""
    a = synth.random_soup(100, seed=5, tri_size=0.12, textures=synth.procedural_textures(32, 9)).meshes[0]
    b = synth.random_soup(60, seed=6, tri_size=0.12).meshes[0]
    a.bbox_min = a.bbox_max = b.bbox_min = b.bbox_max = None
    b.name, b.base_color = "soup_1", (0.3, 0.9, 0.5, 1.0)
    scene = Scene([a, b])
    R = 128
    cnt = oracle.count_per_triangle(scene, R)
    assert cnt[98] > 0 and cnt[100] > 0 and cnt[98:101].sum() < 64     # fragments on both sides of the boundary, less than a strip apart
    check(oracle, scene, R)


def test_deferred_triangle_and_a_cap_inside_a_strip(hiplib, oracle):
    """One triangle too large for the workgroup (deferred to k_emit_big: the workgroup's strips take the irregular path through
    tskip) and a cap that ends the output in the middle of a strip behind it."""
    s = synth.random_soup(300, seed=21, tri_size=0.1, textures=synth.procedural_textures(16, 2))
    v = s.meshes[0].vertices.reshape(300, 3, -1).copy()
    v[150, :, 0:3] = np.float32([[0.2, 0.2, 0.5], [0.7, 0.25, 0.5], [0.3, 0.75, 0.55]])
    scene = Scene([Mesh("big", v.reshape(-1, v.shape[2]), base_color=(0.8, 0.6, 0.4, 0.9), textures=s.meshes[0].textures)])
    R = 128
    cnt = oracle.count_per_triangle(scene, R).astype(np.int64)
    assert cnt[150] > 500 and cnt.sum() - cnt[150] > 500
    full = check(oracle, scene, R)
    assert full == cnt.sum()
    cap = int(cnt[:200].sum()) + 29
    assert cnt[:151].sum() + 64 < cap < full - 64
    check(oracle, scene, R, cap=cap)


def overflow_scene(R):
    """174 080 triangles of one fragment each on a grid of two pixels' pitch (enough triangles for 64-triangle batches: a workgroup is
    256 consecutive triangles) — except workgroup 300, whose 256 triangles have legs of 7.4 pixels: 21 fragments each in 8 x 8 boxes."""
    px = 1.0 / R
    n = 680 * 256
    idx = np.arange(n)
    tris = right_triangles(np.stack([(2 * (idx % 512) + 0.1) * px, (2 * (idx // 512) + 0.1) * px], axis=1), 1.5 * px)
    k = np.arange(256)
    tris[256 * 300:256 * 301] = right_triangles(np.stack([(9 * (k % 100) + 0.55) * px, (700 + 9 * (k // 100) + 0.55) * px], axis=1), 7.4 * px)
    return Scene([Mesh("overflow", flat_triangles(tris), textures=synth.procedural_textures(64, 7), **UNIT_BOX)])


def test_entry_overflow_demotes_and_returns_the_same_bytes(hiplib, oracle):
    """One workgroup's triangles all fit 8 x 8 boxes but hold 256 x 21 = 5376 fragments, more than the 4096 entries of the stream:
    k_fused3 reports the overflow, the library answers with the next forms of the ladder (k_fused2 keeps 4096 entries as well: the
    multi-pass pipeline) and says so."""
    R = 1024
    scene = overflow_scene(R)
    cnt = oracle.count_per_triangle(scene, R)
    sel = slice(256 * 300, 256 * 301)
    assert np.all(cnt[sel] == 21) and np.all(np.delete(cnt, np.arange(sel.start, sel.stop)) == 1)
    check(oracle, scene, R, expect="multipass")


def test_triangle_range_with_an_odd_start_and_a_partial_last_batch(hiplib, oracle):
    scene = synth.cube_sphere(24, tex_size=64)
    check(oracle, scene, 160, tri_range=(101, 2999))
