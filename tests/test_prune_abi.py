"""CPU: the symbols, struct sizes and NULL / no-device handling of the contribution pass and the pruning (no compute calls)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from mesh2splat_amd import _lib
from mesh2splat_amd.prune import DEFAULT_ELEVATIONS, PruneParamsC, orbit_cameras
from mesh2splat_amd.splat import SplatParamsC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m2s_device_sorted_sources", "m2s_download_sorted_sources", "m2s_upload_quad_sources", "m2s_contrib_begin", "m2s_contrib_accumulate", "m2s_device_contrib",
       "m2s_download_contrib", "m2s_last_contrib_ms", "m2s_last_contrib_stage_ms", "m2s_prune", "m2s_last_prune_counts", "m2s_last_prune_ms")


def test_symbols_exported(hiplib):
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(hiplib, name), name


def test_ctypes_mirror_layout():
    assert C.sizeof(PruneParamsC) == 12 and [getattr(PruneParamsC, f).offset for f, _ in PruneParamsC._fields_] == [0, 4, 8]


def test_struct_layout_matches_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(m2s_prune_params), '
                   'offsetof(m2s_prune_params, min_pixels), offsetof(m2s_prune_params, reserved), sizeof(m2s_splat_params));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [12, 4, 8, C.sizeof(SplatParamsC)]


def test_null_context(hiplib):
    """Every entry point refuses a NULL context (what a caller holds when m2s_create found no device: M2S_ERR_NO_DEVICE)."""
    h = C.c_void_p()
    st = hiplib.m2s_create(0, C.byref(h))
    if st == 0:
        hiplib.m2s_destroy(h)
    else:
        assert st == 2 and not h.value
    sp, pp = SplatParamsC(), PruneParamsC(0.0, 0, 0)
    out4, out3, kept = (C.c_uint64 * 4)(), (C.c_float * 3)(), C.c_uint64()
    assert hiplib.m2s_contrib_begin(None) == 1
    assert hiplib.m2s_contrib_accumulate(None, C.byref(sp), C.c_float(0.0)) == 1
    assert hiplib.m2s_upload_quad_sources(None, None, 0) == 1
    assert hiplib.m2s_download_contrib(None, None, None, 0) == 1 and hiplib.m2s_download_sorted_sources(None, None, 0) == 1
    assert hiplib.m2s_prune(None, C.byref(pp), C.byref(kept)) == 1
    assert hiplib.m2s_last_prune_counts(None, out4) == 1 and hiplib.m2s_last_contrib_stage_ms(None, out3) == 1
    assert hiplib.m2s_device_sorted_sources(None) is None and hiplib.m2s_device_contrib(None, 0) is None
    assert hiplib.m2s_last_contrib_ms(None) == 0.0 and hiplib.m2s_last_prune_ms(None) == 0.0


def test_orbit_cameras_over_elevations():
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    cams = orbit_cameras(box, 4, 64, 48, (-30.0, 0.0, 45.0))
    assert len(cams) == 12 and len(orbit_cameras(box, 2, 64, 48)) == 2 * len(DEFAULT_ELEVATIONS)
    ys = [c.eye[1] for c in cams]
    assert all(y < 0 for y in ys[:4]) and all(abs(y) < 1e-12 for y in ys[4:8]) and all(y > 0 for y in ys[8:])
    with pytest.raises(ValueError):
        orbit_cameras(box, 2, 64, 48, ())
    with pytest.raises(ValueError):
        orbit_cameras(box, 2, 64, 48, (90.0,))
