"""-m gpu: the dispatch order that deals the runs to the eight XCD queues by weight (launch_run_order, m2s_run_balance.h) changes WHEN a
run is converted, never what it writes or where — for k_fused3 (lean), k_fused2 (team) and k_sparse, which all read the one table.

Scenes: the smallest cube-spheres that are launched in runs and leave a ragged last group of eight — n = 148 (1027 units of 256
triangles, 33 runs of 32: one run past four full groups) and n = 162 (1231 units, 39 runs: one short of five groups) — and the two
co-located spheres of tests/test_gpu_fused3_stagger.py, whose light runs are several times lighter than the heavy ones, under the sparse
form (units of 512 triangles, runs of 16).

Every case converts on a FRESH context at R = 512 (the first conversion, then a repeated one) and at R = 488 (a launch without runs that
leaves the run table, then one that reads it under the order built at the first density); the counter and all records must equal, byte
for byte, those of a fresh context forced to the multi-pass pipeline, computed once per (scene, R).  At these densities the sparse form
overflows its stream on the large sphere and hands the launch to the team kernel, so the skewed scene runs once more at R = 256 and 240,
where k_sparse itself converts it.
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
        if name == "skewed":
            tex = synth.procedural_textures(256)
            s = Scene([Mesh(name=f"sphere_{k}", vertices=synth.cube_sphere_vertices(105, radius=r), base_color=(1.0, 1.0, 1.0, 1.0), textures=tex)
                       for k, r in enumerate((1.0, 0.35))])           # 2 x 132 300 triangles = 1034 units of 256, 517 of 512
        else:
            s = synth.cube_sphere(int(name), tex_size=256)            # 148: 262 848 triangles = 1027 units; 162: 314 928 = 1231 units
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


def same_bytes(c, total, name, R, what, pipeline):
    rtotal, rrec = reference(name, R)
    rec = c.download().view(np.uint32)
    print(f"{name} R={R} {what}: ran {c.last_pipeline}, {total} Gaussians, multi-pass {rtotal}")
    if pipeline is not None:
        assert c.last_pipeline == pipeline, (what, c.last_pipeline)
    assert total == rtotal and rec.shape == rrec.shape, (what, total, rtotal, rec.shape, rrec.shape)
    assert np.array_equal(rec, rrec), "%s: first differing record %d" % (what, int(np.flatnonzero((rec != rrec).any(axis=1))[0]))


def four_conversions(name, pipeline, expect, R=512, R2=488):
    with Converter(0) as c:
        c.set_pipeline(pipeline)
        c.upload_scene(scene_of(name))
        c.set_max_gaussians(0)
        same_bytes(c, c.convert(R), name, R, "first conversion of the context", expect)
        same_bytes(c, c.convert(R), name, R, "repeated conversion", expect)
        same_bytes(c, c.convert(R2), name, R2, "first conversion at a new density (leaves the run table)", expect)
        same_bytes(c, c.convert(R2), name, R2, "second conversion at the new density (reads that run table)", expect)


@pytest.mark.parametrize("pipeline", ["lean", "team"])
@pytest.mark.parametrize("name,units", [("148", 1027), ("162", 1231)])
def test_ragged_last_group_same_bytes_as_multipass(hiplib, name, units, pipeline):
    scene = scene_of(name)
    assert (scene.n_triangles + 255) // 256 == units and ((units + 31) // 32) % 8 != 0
    four_conversions(name, pipeline, pipeline)


def test_skewed_sparse_same_bytes_as_multipass(hiplib):
    # (at these densities the large sphere's workgroups overflow k_sparse's stream and the launch is repeated by the team kernel: the
    # bytes must match whichever kernel ends up writing them)
    four_conversions("skewed", "sparse", None)


def test_skewed_sparse_kernel_same_bytes_as_multipass(hiplib):
    # a quarter of the fragments: about one per triangle on the large sphere, k_sparse itself reads the table
    four_conversions("skewed", "sparse", "sparse", 256, 240)
