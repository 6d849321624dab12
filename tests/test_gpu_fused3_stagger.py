"""-m gpu: k_fused3's wave priorities (the triangle phase ahead of the strips; in A/B builds a priority per phase class) and the dispatch
order of the runs (k_run_order; in A/B builds with a first resident set of heavy and light runs side by side) change WHEN a workgroup
does its work, never what it writes or where.

Every case converts a scene on a FRESH context whose first conversion is the launch under test (no records of an earlier pipeline
in the buffer that could stand in for a run that was never dispatched) and compares the counter and all stored records byte for
byte with a second fresh context forced to the multi-pass pipeline; then again for a repeated conversion (the asynchronous fast
path), and for a density the context has never seen: its first launch there runs without runs and leaves the run table, the second
one reads that table — under the dispatch order built at the first density.

Scenes: the smallest cube-sphere that is launched in runs (n = 148: 1027 units of 256 triangles, runs of 32), two co-located spheres
of different radius (the runs of the small one are several times lighter: a spread order is far from the identity, and an order that
is no permutation loses or repeats a run), and the CI-sized sphere, which launches without runs.  The multi-pass reference of a (scene, R) is computed once.
"""
import numpy as np
import pytest

from mesh2splat_amd import synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.scene import Mesh, Scene

pytestmark = pytest.mark.gpu

_scenes, _reference = {}, {}


def scene_of(name):
    if name not in _scenes:
        if name == "runs":
            s = synth.cube_sphere(148, tex_size=256)                  # 262 848 triangles = 1027 units: run_shift_for -> 5
        elif name == "skewed":
            tex = synth.procedural_textures(256)
            s = Scene([Mesh(name=f"sphere_{k}", vertices=synth.cube_sphere_vertices(105, radius=r), base_color=(1.0, 1.0, 1.0, 1.0), textures=tex)
                       for k, r in enumerate((1.0, 0.35))])           # 2 x 132 300 triangles = 1034 units
        else:
            s = synth.cube_sphere(24, tex_size=256)                   # 6 912 triangles: batches below 64 triangles, no runs
        _scenes[name] = s
    return _scenes[name]


def reference(name, R):
    """(counter, records as uint32) of the multi-pass pipeline on a fresh context"""
    if (name, R) not in _reference:
        with Converter(0) as c:
            c.set_pipeline("multipass")
            c.upload_scene(scene_of(name))
            c.set_max_gaussians(0)
            total = c.convert(R)
            assert c.last_pipeline == "multipass"
            rec = c.download().view(np.uint32).copy()
            rec.setflags(write=False)
            _reference[(name, R)] = (total, rec)
    return _reference[(name, R)]


def same_bytes(c, total, name, R, what):
    rtotal, rrec = reference(name, R)
    assert c.last_pipeline == "lean", (what, c.last_pipeline)
    rec = c.download().view(np.uint32)
    print(f"{name} R={R} {what}: {total} Gaussians, multi-pass {rtotal}")
    assert total == rtotal and rec.shape == rrec.shape, (what, total, rtotal, rec.shape, rrec.shape)
    assert np.array_equal(rec, rrec), "%s: first differing record %d" % (what, int(np.flatnonzero((rec != rrec).any(axis=1))[0]))


@pytest.mark.parametrize("name,pipeline,R,R2", [("runs", "auto", 512, 488), ("skewed", "auto", 512, 488), ("small", "lean", 160, 152)])
def test_same_bytes_as_multipass(hiplib, name, pipeline, R, R2):
    scene = scene_of(name)
    if name != "small":
        assert scene.n_triangles >= 1024 * 256
    with Converter(0) as c:
        c.set_pipeline(pipeline)
        c.upload_scene(scene)
        c.set_max_gaussians(0)
        same_bytes(c, c.convert(R), name, R, "first conversion of the context")
        same_bytes(c, c.convert(R), name, R, "repeated conversion")
        same_bytes(c, c.convert(R2), name, R2, "first conversion at a new density (leaves the run table)")
        same_bytes(c, c.convert(R2), name, R2, "second conversion at the new density (reads that run table)")


def test_skewed_scene_has_skewed_runs(hiplib):
    """the premise of the "skewed" case: its light runs (the small sphere's) hold several times fewer fragments than its heavy ones"""
    scene = scene_of("skewed")
    with Converter(0) as c:
        c.upload_scene(scene)
        c.convert(512)
        cnt = c.download_triangle_counts().astype(np.int64)
    per_run = np.add.reduceat(cnt, np.arange(0, len(cnt), 256 * 32))
    assert len(per_run) >= 32 and per_run.max() > 3 * per_run.min(), (per_run.min(), per_run.max())
