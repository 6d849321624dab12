"""-m gpu: a context that has grown gives the bytes of a fresh one.

The viewer passes keep grow-only work buffers in the context and slice some of them by their CAPACITY, others by the current size.  A
slice that is wrong only when the capacity exceeds the size cannot be seen by a test that runs one size per context, so this one runs
the same sequence of passes through ONE Converter at a small configuration, a large one and the small one again, and compares every
output it can download, byte for byte, with the same sequence in a fresh Converter at that configuration alone.

Every pass involved is order-independent (integer min / max / add atomics, array-order blending, stable sorts): equality is exact.
Nothing here is anchored to the code under test - each pass is held to its reference by its own test; this asserts independence from
the context's history only."""
from dataclasses import replace

import numpy as np
import pytest

import camera
from mesh2splat_amd import synth
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prepass import PrepassParams
from mesh2splat_amd.splat import SplatParams

pytestmark = pytest.mark.gpu

#          cube_sphere, R, frame (W, H), shadow cube
SMALL = (4, 16, (64, 48), 64)
LARGE = (12, 64, (320, 200), 256)
EYE, AT = (1.6, 1.1, 2.3), (0.1, 0.0, -0.1)
NEAR, FAR = 0.01, 100.0


def run_sequence(conv, cfg):
    """The passes of one viewer session at `cfg` -> {name: array} of everything downloaded on the way."""
    n_sphere, R, (W, H), S = cfg
    out = {}
    conv.upload_scene(synth.cube_sphere(n_sphere))
    out["stored"] = np.array([conv.convert(R)])
    out["records"] = conv.download()
    view = camera.look_at(EYE, AT)
    pp = PrepassParams(view_mat=view, proj_mat=camera.perspective(45.0, W / H, NEAR, FAR), renderer_resolution=(W, H), near_plane=NEAR,
                       far_plane=FAR, resolution_target=R, render_mode=6)
    lp = LightParams(light_position=(0.5, 1.5, 3.0), camera_position=EYE, near_plane=NEAR, far_plane=FAR, renderer_resolution=(W, H),
                     shadow_resolution=S, want_shadow_counts=True)
    # depth sort of the records
    out["sorted_n"] = np.array([conv.sort_by_depth(view.T, download=False)])
    out["sorted"] = conv.download_sorted()
    # prepass + sort of its survivors; the same frame as one pass (no depth image: the dense path, sources = the permutation)
    vis, quads, depths = conv.prepass(pp)
    out["quads"], out["depths"] = quads, depths
    out["sorted_quads"] = conv.sort_prepass()
    out["sorted_quads_dense"] = conv.prepass_sorted(pp)
    out["sources_dense"] = conv.download_sorted_sources(len(out["sorted_quads_dense"]))
    # one frame with the mesh as occluder and the split screen: mesh depth, compacting prepass_sorted, splat, shadow, mesh render, split
    frame, counts = conv.render_frame(pp, lp, mesh_depth_test=True, split_screen=0.5)
    out["frame_split"], out["shadow_counts_split"] = frame, counts
    out["mesh_depth"] = conv.download_mesh_depth()
    for k, plane in enumerate(conv.download_gbuffer()):
        out[f"gbuffer{k}"] = plane
    for k, plane in enumerate(conv.download_mesh_gbuffer()):
        out[f"mesh_gbuffer{k}"] = plane
    out["mesh_visibility"] = conv.download_mesh_visibility()
    out["shadow_cube"] = conv.download_shadow_cubemap()
    out["frame"], out["shadow_counts"] = conv.relight(lp)
    # the compacting path's quads and sources (what render_frame drew), then what every record adds to that picture
    out["sorted_quads_compact"] = conv.prepass_sorted(conv._with_device_mesh_depth(pp))
    out["sources_compact"] = conv.download_sorted_sources(len(out["sorted_quads_compact"]))
    conv.contrib_begin()
    conv.contrib_accumulate(SplatParams((W, H), 0))
    wmax, npix = conv.download_contrib()
    out["contrib_wmax"], out["contrib_npix"] = wmax.view(np.uint32), npix
    # the light baked into the coefficient plane, then the records nobody sees go (the plane is compacted with them)
    sh, taps = conv.bake_light(BakeParams(want_shadow_counts=True), lp)
    out["sh"], out["bake_counts"] = sh, taps
    out["prune_counts"] = np.array(list(conv.prune(0.0, 0).values()))
    out["pruned_records"] = conv.download()
    out["pruned_sh"] = conv.download_sh()
    # the session is no empty one: something is drawn, something is pruned away, something stays
    assert vis > 0 and len(out["sorted_quads_compact"]) > 0 and 0 < len(out["pruned_records"]) < len(out["records"])
    return out


@pytest.fixture(scope="module")
def runs(hiplib):
    fresh = {}
    for name, cfg in (("small", SMALL), ("large", LARGE)):
        with Converter(0) as c:
            fresh[name] = run_sequence(c, cfg)
    with Converter(0) as c:
        reused = [(name, run_sequence(c, cfg)) for name, cfg in (("small", SMALL), ("large", LARGE), ("small", SMALL))]
    assert len(fresh["large"]["records"]) > 4 * len(fresh["small"]["records"])       # the context really grows, then runs below capacity
    return fresh, reused


@pytest.mark.parametrize("step", [0, 1, 2], ids=["small_first", "large_after_small", "small_after_large"])
def test_reused_context_equals_fresh_context(runs, step):
    fresh, reused = runs
    name, got = reused[step]
    want = fresh[name]
    assert sorted(got) == sorted(want)
    bad = []
    for key in sorted(want):
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        same = a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
        if not same:
            bad.append(f"{key}: shape {a.shape} / {b.shape}, bytes that differ "
                       f"{int((a.view(np.uint8) != b.view(np.uint8)).sum()) if a.shape == b.shape else 'n/a'}")
    print(f"{name} (step {step}): {len(want)} outputs, {sum(np.asarray(v).nbytes for v in want.values())} bytes compared, "
          f"{len(want['records'])} records, {len(want['sorted_quads_compact'])} quads drawn, {len(want['pruned_records'])} kept")
    assert not bad, "; ".join(bad)
