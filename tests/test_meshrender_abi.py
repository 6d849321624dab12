"""The C ABI of the mesh render pass and the split-screen relighting: include/m2s.h declares the entry points, mesh2splat_amd/_lib.py
binds them with the declared signatures, and the ctypes mirror of the parameter struct has the header's layout.  No GPU."""
import ctypes as C
import os
import re

from mesh2splat_amd import _lib
from mesh2splat_amd.meshrender import COUNT_NAMES, STAGE_NAMES, MeshRenderParamsC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("m2s_mesh_render", "m2s_device_mesh_gbuffer", "m2s_download_mesh_gbuffer", "m2s_download_mesh_visibility",
                "m2s_last_mesh_render_ms", "m2s_last_mesh_render_stage_ms", "m2s_last_mesh_render_counts", "m2s_relight_split")


def test_header_declares_and_lib_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "m2s.h")).read()
    L = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), f"{name} is not declared in include/m2s.h"
        assert name in _lib.EXPORTS, f"{name} is not listed in _lib.EXPORTS"
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is not None, f"{name} has no prototype"
    assert L.m2s_relight_split.argtypes[-1] is C.c_float and L.m2s_last_mesh_render_ms.restype is C.c_float
    body = re.search(r"typedef struct m2s_mesh_render_params \{(.*?)\} m2s_mesh_render_params;", header, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[\d+\])?(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in MeshRenderParamsC._fields_]
    assert C.sizeof(MeshRenderParamsC) == 3 * 64 + 24
    assert len(COUNT_NAMES) == 6 and len(STAGE_NAMES) == 4
    # NULL handles are rejected before anything touches a device
    assert L.m2s_mesh_render(None, None, None) == 1 and L.m2s_relight_split(None, None, 0.5) == 1
    assert L.m2s_device_mesh_gbuffer(None, 0) is None and L.m2s_last_mesh_render_ms(None) == 0.0
