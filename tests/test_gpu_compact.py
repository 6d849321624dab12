"""-m gpu: m2s_export_ply_compact / Converter.export_ply_compact — the device's file against m2s_write_ply_compact on the downloaded
records and against the numpy restatement (tests/compact_ref.py), byte for byte: uploaded record sets with every edge of the pin, 70 000
random records, a real conversion with and without the position plane, after pruning, with baked planes; what the export must leave
untouched; the error paths."""
import ctypes as C
import os

import numpy as np
import pytest

import camera
import compact_ref as cr
from mesh2splat_amd import synth
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter, write_ply_compact
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prune import orbit_cameras
from mesh2splat_amd.scene import Mesh, Scene
from mesh2splat_amd.splat import SplatParams

pytestmark = pytest.mark.gpu
R, W, H = 64, 128, 128
STD = 0.65


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def sphere():
    return Scene([Mesh(name="sphere", vertices=synth.cube_sphere_vertices(10, 1.0), base_color=(0.8, 0.6, 0.4, 1.0))])


def check(conv, tmp_path, rec, sm, sh=None, degree=0, restate=True, std=STD):
    """the device's file == the host writer's on `rec` (== the restatement's); -> the bytes"""
    dev, host = str(tmp_path / "dev.ply"), str(tmp_path / "host.ply")
    got = conv.export_ply_compact(dev, std, baked_sh=sh is not None)
    want = write_ply_compact(host, rec, sm, sh, degree)
    a, b = open(dev, "rb").read(), open(host, "rb").read()
    assert {k: got[k] for k in want} == want and got["bytes"] == len(a)
    if a != b:
        ha, ta, ra, sa = cr.parse(a)
        hb, tb, rb, sb = cr.parse(b)
        print("header", ha == hb, "table rows differing", np.argwhere((ta.view(np.uint32) != tb.view(np.uint32)).any(1))[:8].ravel(),
              "vertex rows differing", np.argwhere((ra != rb).any(1))[:8].ravel(), "sh rows differing", np.argwhere((sa != sb).any(1))[:8].ravel())
    assert a == b
    if restate:
        ref, counts, _ = cr.encode(rec, sm, sh, degree)
        assert a == ref and counts == want
    return a


@pytest.mark.parametrize("name", list(cr.cases()))
def test_uploaded_cases(conv, tmp_path, name):
    rec, sm = cr.cases()[name]
    conv.upload_records(rec)
    check(conv, tmp_path, rec, np.float32(sm), std=sm)          # uploaded records carry no resolutionTarget: sm = gaussian_std


def test_many_workgroups(conv, tmp_path):
    rec = cr.hostile(cr.make_records(70000, 11, spread=3.0))
    conv.upload_records(rec)
    a = check(conv, tmp_path, rec, np.float32(0.01), std=0.01)
    assert check(conv, tmp_path, rec, np.float32(0.01), std=0.01, restate=False) == a       # two calls in a row


def test_conversion_plane_prune_bake(conv, tmp_path):
    scene = sphere()
    conv.upload_scene(scene)
    n = conv.convert(R)
    assert 8000 < n < 20000
    rec = conv.download()
    sm = np.float32(STD) / np.float32(R)
    assert not conv.positions_ready
    a = check(conv, tmp_path, rec, sm)
    conv.sort_by_depth(camera.look_at((1.6, 1.1, 2.3), (0.1, 0.0, -0.1)), download=False)      # leaves the 16-byte position plane behind
    assert conv.positions_ready
    assert check(conv, tmp_path, rec, sm, restate=False) == a
    assert np.array_equal(conv.download().view(np.uint32), rec.view(np.uint32))
    for degree in (1, 3):
        sh = conv.bake_light(BakeParams(degree=degree, use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)))
        b = check(conv, tmp_path, rec, sm, sh, degree)
        assert b"element sh" in b[:4096] and f"f_rest_{3 * ((degree + 1) ** 2 - 1) - 1}\n".encode() in b[:4096]
        assert np.array_equal(conv.download_sh().view(np.uint32), sh.view(np.uint32))
    counts = conv.prune_views(orbit_cameras(scene, 2, W, H, (20.0,)), R)
    assert 0 < counts["kept"] < n
    kept, sh_kept = conv.download(), conv.download_sh()
    check(conv, tmp_path, kept, sm)
    check(conv, tmp_path, kept, sm, sh_kept, 3)


def test_leaves_the_context_alone(conv, tmp_path):
    scene = sphere()
    conv.upload_scene(scene)
    n = conv.convert(R)
    rec = conv.download()
    sh = conv.bake_light(BakeParams(degree=2, use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)))
    pp, _ = orbit_cameras(scene, 1, W, H, (20.0,))[0].frame_params(R, (0, 0, 0), 0.0)
    conv.contrib_begin()
    nq = conv.prepass_sorted(pp, download=False)
    assert nq > 0 and conv.device_sorted_sources
    conv.contrib_accumulate(SplatParams((W, H), 0), 1.0 / 255.0)
    src, (w, k) = conv.download_sorted_sources(nq), conv.download_contrib()
    def sorted_quads():
        out = np.empty((nq, 24), np.float32)
        conv._check(conv._L.m2s_download_sorted_quads(conv._h, out.ctypes.data, nq))
        return out
    quads = sorted_quads()
    ptr = conv.device_records
    conv.export_ply_compact(str(tmp_path / "a.ply"), STD, baked_sh=True)
    assert conv.device_records == ptr and conv.num_stored == n and conv.device_sorted_sources
    assert np.array_equal(conv.download_sorted_sources(nq), src)
    w2, k2 = conv.download_contrib()
    assert np.array_equal(w2.view(np.uint32), w.view(np.uint32)) and np.array_equal(k2, k)
    assert np.array_equal(conv.download_sh().view(np.uint32), sh.view(np.uint32))
    assert np.array_equal(conv.download().view(np.uint32), rec.view(np.uint32))
    assert np.array_equal(sorted_quads().view(np.uint32), quads.view(np.uint32))


def test_error_paths(hiplib, tmp_path):
    c = Converter(0)
    try:
        path = os.fsencode(str(tmp_path / "never.ply"))
        counts = (C.c_uint64 * 3)()
        L, h = c._L, c._h
        assert L.m2s_export_ply_compact(None, path, C.c_float(0.65), 0, counts) == 1
        assert L.m2s_export_ply_compact(h, None, C.c_float(0.65), 0, counts) == 1
        assert L.m2s_export_ply_compact(h, path, C.c_float(0.65), 0, counts) == 7                # no records
        c.upload_records(cr.make_records(300, 1))
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert L.m2s_export_ply_compact(h, path, C.c_float(bad), 0, counts) == 1
        assert L.m2s_export_ply_compact(h, path, C.c_float(0.65), 1, counts) == 7                # no baked plane
        c.bake_light(BakeParams(degree=1, use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)))
        assert L.m2s_export_ply_compact(h, path, C.c_float(0.65), 1, counts) == 0
        c.upload_records(cr.make_records(200, 2))
        assert L.m2s_export_ply_compact(h, path, C.c_float(0.65), 1, counts) == 7                # a plane of another count
        assert L.m2s_export_ply_compact(h, os.fsencode(str(tmp_path / "no" / "dir.ply")), C.c_float(0.65), 0, counts) == 6
        assert L.m2s_export_ply_compact(h, path, C.c_float(0.65), 0, None) == 0                  # counts are optional
        ms = (C.c_float * 4)()
        assert L.m2s_last_compact_stage_ms(h, ms) == 0 and L.m2s_last_compact_stage_ms(None, ms) == 1 and ms[3] > 0
    finally:
        c.close()
