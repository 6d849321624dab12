"""-m gpu: m2s_device_sorted_sources after m2s_prepass_sorted — the values, on both of its paths.  Dense (no depth image: the sources
are the head of the sort's permutation) and compacting (a depth image, or a survivor whose depth bits are the culled marker: k_prepass
stores the record index beside the quad).  Against the oracle's prepass: sorted quad i must be, bit for bit, the oracle's prepass of
record sources[i]; the sources are distinct record indices, as many as the oracle's survivors, in the order of a stable sort by depth."""
import numpy as np
import pytest

import prepass_cases
from mesh2splat_amd.converter import Converter

pytestmark = pytest.mark.gpu
CASES = dict(prepass_cases.cases())


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_sources(conv, oracle, p, rec, what):
    conv.upload_records(rec)
    quads = conv.prepass_sorted(p)
    wk, _, _ = oracle.prepass(p, rec)
    assert quads.shape[0] == wk > 0, what
    assert conv.device_sorted_sources, what
    src = conv.download_sorted_sources(wk)
    # a strictly valid subset: indices of records, none twice, as many as survive
    assert src.max() < rec.shape[0] and np.unique(src).size == wk, what
    # quad i is the prepass of record src[i]: the oracle over the records gathered in that order keeps every one of them, in order
    gk, gq, gd = oracle.prepass(p, rec[src])
    assert gk == wk, f"{what}: {wk - gk} sourced records do not survive the oracle's prepass"
    same = (bits(gq) == bits(quads)) | (np.isnan(gq) & np.isnan(quads))
    assert same.all(), f"{what}: quads differ from their sources' at {np.argwhere(~same)[:4].tolist()}"
    # depth order, and record order among equal depths (the duplicated records: a stable sort)
    key = gd.view(np.uint32).astype(np.int64)
    assert ((np.diff(key) > 0) | ((np.diff(key) == 0) & (np.diff(src.astype(np.int64)) > 0))).all(), what
    return src


@pytest.mark.parametrize("name", ["colour", "inside", "depth_test"])
def test_sources_name_the_record_of_every_sorted_quad(conv, oracle, name):
    """"colour", "inside" (most records culled): the dense path; "depth_test": the compacting path."""
    p = CASES[name]
    rec = np.concatenate([prepass_cases.base_records(oracle, 14, 64), prepass_cases.hostile_records(2048)])[:-13]
    rec = np.concatenate([rec, rec[:3000]])
    src = check_sources(conv, oracle, p, rec, name)
    assert src.size < rec.shape[0] and not np.array_equal(src, np.sort(src))          # (a subset, and not in record order)
    # a second frame through the same context: the sources are this frame's
    from dataclasses import replace
    view, proj = prepass_cases.default_camera((800, 450))
    check_sources(conv, oracle, replace(p, view_mat=view, proj_mat=proj, renderer_resolution=(800, 450),
                                        mesh_depth=prepass_cases.depth_image((800, 450)) if p.perform_mesh_depth_test else p.mesh_depth), rec, name + ", frame 2")


def test_sources_when_a_survivors_depth_bits_are_the_culled_marker(conv, oracle):
    """The marker clash of tests/test_gpu_prepass.py: no depth image, yet the prepass compacts."""
    rec = prepass_cases.base_records(oracle, 12, 64).copy()
    allones = np.array([0xFFFFFFFF], np.uint32).view(np.float32)[0]
    rec[5::97, 0] = allones
    rec[7::131, 2] = allones
    check_sources(conv, oracle, CASES["colour"], rec, "marker clash")


def test_sources_through_the_device_mesh_depth_image(conv, oracle):
    """The frame's own way to the compacting path: the mesh depth prepass of the uploaded scene, tested against on the device."""
    from mesh2splat_amd import synth
    from dataclasses import replace
    scene = synth.cube_sphere(12)
    R = 48
    conv.upload_scene(scene)
    n = conv.convert(R)
    rec = conv.download()
    p = replace(CASES["colour"], resolution_target=R)
    depth, _ = conv.mesh_depth(p)
    visible = conv.prepass_sorted(conv._with_device_mesh_depth(p), download=False)
    assert 0 < visible < n
    src = conv.download_sorted_sources(visible)
    quads = np.empty((visible, 24), np.float32)
    conv._check(conv._L.m2s_download_sorted_quads(conv._h, quads.ctypes.data, visible))
    ph = replace(p, perform_mesh_depth_test=True, mesh_depth=np.ascontiguousarray(depth, np.float32))
    wk, _, _ = oracle.prepass(ph, rec)
    gk, gq, _ = oracle.prepass(ph, rec[src])
    assert wk == gk == visible and np.unique(src).size == visible
    assert np.array_equal(bits(gq), bits(quads))
