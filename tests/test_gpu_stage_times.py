"""-m gpu: what every stage-time getter of the C ABI reports, pass by pass and situation by situation.

A literal table of (pass, situation, expectation), read off the host code of each pass and not computed from the library under test.
The inputs are the smallest that reach each branch: 257 crafted records (merge_ref.crafted_records) and 0 records, a 64 x 48 viewport,
synth.unit_quad() converted at R = 16 for the conversions and the mesh passes, a tree built with the chain (3, 10), a shadow cube of
side 64.  Expectations:
    POS    finite and > 0: a kernel ran between the two marks
    ZERO   exactly 0.0: the span was not measured in this call (and the pass zeroes or rewrites the value)
    GE0    finite and >= 0: a span around work that can be empty, or around nothing but the marks themselves
Relations between getters are asserted in fp32, with the parenthesisation of the host code.

The three policies:
    gated      most passes: with profiling off a call leaves its getters bit for bit as they were
    always     m2s_merge, m2s_lod_build, m2s_export_ply_compact measure whatever m2s_set_profiling says
    resetting  two gated passes still write without profiling: a conversion zeroes m2s_last_kernel_ms when it starts, and
               m2s_records_to_world_units (on records with R > 1) zeroes m2s_last_world_units_ms

Rows that differ from what one might expect, kept as the code has them:
    * m2s_merge that applies (not a dry run) and finds nothing to merge still runs its reduction: [2] > 0.  [2] == 0 exactly on a dry
      run, on 0 records, and for the step of m2s_lod_build that merges nothing (MergeMode::IfAny turns dry).
    * an unprofiled conversion zeroes m2s_last_kernel_ms (run_pass clears it before it looks at the switch).
    * m2s_splat over quads that give no pairs: [0] is the setup alone (> 0), [1] a span around nothing (>= 0), [2] the blend, which
      still writes the cleared planes (> 0).
    * m2s_shadow on 0 records: three zeros and a total of 0; on records none of which reaches a face: [0] is the counting kernel
      (> 0), [1] == [2] == 0.
    * m2s_mesh_depth with a deferred triangle that gives no pairs: the clipper's span is closed by a mark of its own, [1] > 0, [2] == 0.
Passes left out: none."""
import ctypes as C
import math

import numpy as np
import pytest

import camera
import merge_ref as mr
from mesh2splat_amd import lod as _ld, synth
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prepass import PrepassParams
from mesh2splat_amd.refit import RefitParams
from mesh2splat_amd.score import ScoreParams
from mesh2splat_amd.splat import SplatParams

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 64, 48
S = 64
POS, ZERO, GE0 = "POS", "ZERO", "GE0"

# name -> (C getter, entries; 0: the getter returns the float itself)
GETTERS = {
    "kernel": ("m2s_last_kernel_ms", None),          # M2S_K_N entries: sized from the wrapper below
    "sort": ("m2s_last_sort_ms", 0), "sort_stage": ("m2s_last_sort_stage_ms", 3),
    "prepass": ("m2s_last_prepass_ms", 0), "sort_prepass": ("m2s_last_sort_prepass_ms", 0),
    "splat": ("m2s_last_splat_ms", 0), "splat_stage": ("m2s_last_splat_stage_ms", 3),
    "contrib": ("m2s_last_contrib_ms", 0), "contrib_stage": ("m2s_last_contrib_stage_ms", 3),
    "prune": ("m2s_last_prune_ms", 0), "budget_stage": ("m2s_last_budget_stage_ms", 3),
    "refit_stage": ("m2s_last_refit_stage_ms", 3), "refit_apply": ("m2s_last_refit_apply_ms", 0),
    "merge_stage": ("m2s_last_merge_stage_ms", 3), "lod_build": ("m2s_last_lod_build_ms", 0),
    "lod_select_stage": ("m2s_last_lod_select_stage_ms", 3), "lod_budget_stage": ("m2s_last_lod_budget_stage_ms", 3),
    "lod_frustum": ("m2s_last_lod_frustum_ms", 0), "world_units": ("m2s_last_world_units_ms", 0),
    "shadow": ("m2s_last_shadow_ms", 0), "shadow_stage": ("m2s_last_shadow_stage_ms", 3), "relight": ("m2s_last_relight_ms", 0),
    "mesh_depth": ("m2s_last_mesh_depth_ms", 0), "mesh_depth_stage": ("m2s_last_mesh_depth_stage_ms", 3),
    "mesh_render": ("m2s_last_mesh_render_ms", 0), "mesh_render_stage": ("m2s_last_mesh_render_stage_ms", 4),
    "score": ("m2s_last_score_ms", 0), "bake": ("m2s_last_bake_ms", 0), "compact_stage": ("m2s_last_compact_stage_ms", 4),
}
ALWAYS = ("merge_stage", "lod_build", "compact_stage")
RESETTING = ("kernel", "world_units")


def times(L, conv):
    """every time getter -> a tuple of floats (each the exact value of the fp32 the library holds)"""
    out = {}
    for name, (fn, n) in GETTERS.items():
        if name == "kernel":
            out[name] = tuple(conv.last_kernel_ms().values())
        elif n == 0:
            out[name] = (float(getattr(L, fn)(conv._h)),)
        else:
            ms = (C.c_float * n)()
            assert getattr(L, fn)(conv._h, ms) == 0
            out[name] = tuple(float(v) for v in ms)
    return out


def gated(t):
    return {k: v for k, v in t.items() if k not in ALWAYS + RESETTING}


def expect(t, name, *cells):
    got = t[name]
    print(f"    {name}: {got}")
    assert len(got) == len(cells), (name, got, cells)
    for k, (v, cell) in enumerate(zip(got, cells)):
        assert math.isfinite(v), (name, k, got)
        if cell == POS:
            assert v > 0.0, (name, k, got)
        elif cell == ZERO:
            assert v == 0.0, (name, k, got)
        else:
            assert cell == GE0 and v >= 0.0, (name, k, got)


def f32sum(*terms):
    """left to right in fp32"""
    acc = F(terms[0])
    for v in terms[1:]:
        acc = F(acc + F(v))
    return float(acc)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.set_profiling(False)
    c.close()


@pytest.fixture(scope="module")
def rec257():
    return mr.crafted_records(257, 1, invalid=False)


EYE, AT = (0.0, 0.0, 6.0), (0.0, 0.0, 0.0)
QEYE, QAT = (0.5, 0.5, 2.0), (0.5, 0.5, 0.0)                  # in front of synth.unit_quad()


def frame(conv, eye=EYE, at=AT, mode=0):
    return PrepassParams(view_mat=camera.look_at(eye, at), proj_mat=camera.perspective(45.0, W / H, 0.01, 100.0), renderer_resolution=(W, H),
                         resolution_target=max(conv.resolution, 1), render_mode=mode)


def light(eye=EYE, position=(1.5, 2.0, 2.5)):
    return LightParams(light_position=position, camera_position=eye, renderer_resolution=(W, H), shadow_resolution=S)


def focal():
    return _ld.focal_px(camera.perspective(45.0, W / H, 0.01, 100.0), H)


def unchanged_by(L, conv, what, call):
    """`call` with profiling off leaves every gated getter bit for bit as it was"""
    before = times(L, conv)
    conv.set_profiling(False)
    try:
        out = call()
    finally:
        conv.set_profiling(True)
    after = times(L, conv)
    assert gated(after) == gated(before), (what, {k: (before[k], after[k]) for k in gated(before) if before[k] != after[k]})
    return out, before, after


def test_fresh_context(hiplib):
    c = Converter(0)
    try:
        for name, got in times(hiplib, c).items():
            assert all(v == 0.0 for v in got), (name, got)
    finally:
        c.close()


def test_sort_and_prepass(conv, hiplib, rec257):
    L = hiplib
    conv.set_profiling(True)
    conv.upload_records(rec257)
    view = camera.look_at(EYE, AT)
    print("m2s_sort_by_depth, 257 records")
    assert conv.sort_by_depth(view, download=False) == 257
    t = times(L, conv)
    expect(t, "sort", POS)
    expect(t, "sort_stage", POS, POS, POS)
    unchanged_by(L, conv, "sort_by_depth", lambda: conv.sort_by_depth(view, download=False))
    print("m2s_prepass")
    vis = conv.prepass(frame(conv), download=False)
    assert vis > 0
    t2 = times(L, conv)
    expect(t2, "prepass", POS)
    assert t2["sort"] == t["sort"] and t2["sort_stage"] == t["sort_stage"]      # the plain prepass is not the sorted one
    unchanged_by(L, conv, "prepass", lambda: conv.prepass(frame(conv), download=False))
    print("m2s_sort_prepass")
    assert conv.sort_prepass(download=False) == vis
    expect(times(L, conv), "sort_prepass", POS)
    unchanged_by(L, conv, "sort_prepass", lambda: conv.sort_prepass(download=False))
    print("m2s_prepass_sorted")
    assert conv.prepass_sorted(frame(conv), download=False) == vis
    t3 = times(L, conv)
    expect(t3, "sort", POS)
    expect(t3, "sort_stage", POS, POS, POS)
    expect(t3, "prepass", POS)
    assert t3["sort_stage"][2] == t3["prepass"][0]
    unchanged_by(L, conv, "prepass_sorted", lambda: conv.prepass_sorted(frame(conv), download=False))
    print("the plain and the sorted prepass write one getter: an unprofiled call of either behind profiled calls of both writes nothing")
    for first, second in ((conv.prepass, conv.prepass_sorted), (conv.prepass_sorted, conv.prepass)):
        assert first(frame(conv), download=False) == vis and second(frame(conv), download=False) == vis
        expect(times(L, conv), "prepass", POS)
        unchanged_by(L, conv, "second prepass", lambda: second(frame(conv), download=False))
        unchanged_by(L, conv, "first prepass", lambda: first(frame(conv), download=False))
    assert conv.sort_by_depth(view, download=False) == 257                      # (shares the sorted prepass's clock)
    unchanged_by(L, conv, "prepass_sorted behind sort_by_depth", lambda: conv.prepass_sorted(frame(conv), download=False))
    t3 = times(L, conv)
    print("0 records: the three passes return before they measure")
    conv.upload_records(np.zeros((0, 24), F))
    assert conv.sort_by_depth(view, download=False) == 0 and conv.prepass_sorted(frame(conv), download=False) == 0
    assert conv.prepass(frame(conv), download=False) == 0 and conv.sort_prepass(download=False) == 0
    assert gated(times(L, conv)) == gated(t3)


def test_splat_and_contribution(conv, hiplib, rec257):
    import torch
    L = hiplib
    conv.set_profiling(True)
    conv.upload_records(rec257)
    conv.contrib_begin()
    assert conv.prepass_sorted(frame(conv), download=False) > 0
    sp = SplatParams((W, H), 0)
    print("m2s_splat, sorted quads")
    conv.splat(sp, download=False)
    assert conv.last_splat_counts()["pairs"] > 0
    t = times(L, conv)
    expect(t, "splat_stage", POS, POS, POS)
    assert t["splat"][0] == f32sum(f32sum(t["splat_stage"][0], t["splat_stage"][1]), t["splat_stage"][2]) > 0
    unchanged_by(L, conv, "splat", lambda: conv.splat(sp, download=False))
    print("m2s_contrib_accumulate")
    conv.contrib_accumulate(sp)
    t = times(L, conv)
    expect(t, "contrib_stage", POS, POS, POS)
    assert t["contrib"][0] == f32sum(f32sum(t["contrib_stage"][0], t["contrib_stage"][1]), t["contrib_stage"][2]) > 0
    unchanged_by(L, conv, "contrib_accumulate", lambda: conv.contrib_accumulate(sp))
    print("m2s_splat, quads without pairs (every field NaN: skipped by the setup)")
    nanq = torch.full((3, 24), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert conv.splat(sp, quads=nanq, download=False) == 3 and conv.last_splat_counts()["pairs"] == 0
    t = times(L, conv)
    expect(t, "splat_stage", POS, GE0, POS)
    assert t["splat"][0] == f32sum(f32sum(t["splat_stage"][0], t["splat_stage"][1]), t["splat_stage"][2])
    print("m2s_splat, no quads: no setup either")
    empty = torch.empty((0, 24), dtype=torch.float32, device="cuda")
    assert conv.splat(sp, quads=empty, download=False) == 0
    t = times(L, conv)
    expect(t, "splat_stage", GE0, GE0, POS)
    assert t["splat"][0] == f32sum(f32sum(t["splat_stage"][0], t["splat_stage"][1]), t["splat_stage"][2])
    print("m2s_prune")
    conv.prune(-1.0, 0)
    expect(times(L, conv), "prune", POS)
    conv.contrib_begin()
    unchanged_by(L, conv, "prune", lambda: conv.prune(-1.0, 0))
    print("m2s_prune, 0 records: the span closes around the pool's allocation alone")
    conv.upload_records(np.zeros((0, 24), F))
    conv.contrib_begin()
    conv.prune(-1.0, 0)
    expect(times(L, conv), "prune", GE0)


def test_isolation(conv, hiplib, rec257):
    """the splat getters are not disturbed by the passes that used to share its events, nor theirs by it"""
    L = hiplib
    conv.set_profiling(True)
    conv.upload_records(rec257)
    assert conv.prepass_sorted(frame(conv), download=False) > 0
    conv.splat(SplatParams((W, H), 0), download=False)
    mine = ("splat", "splat_stage")
    theirs = ("kernel", "sort", "sort_stage", "prepass", "sort_prepass")
    a = times(L, conv)
    conv.upload_scene(synth.unit_quad())
    assert conv.convert(16) == 256
    assert conv.sort_by_depth(camera.look_at(QEYE, QAT), download=False) == 256
    vis = conv.prepass(frame(conv, QEYE, QAT), download=False)
    assert vis > 0 and conv.sort_prepass(download=False) == vis
    b = times(L, conv)
    assert all(b[k] == a[k] for k in mine), (a, b)
    assert all(any(v > 0 for v in b[k]) for k in theirs), b
    conv.splat(SplatParams((W, H), 0), download=False)
    c = times(L, conv)
    assert all(c[k] == b[k] for k in theirs), (b, c)
    expect(c, "splat_stage", POS, POS, POS)


def test_conversion(conv, hiplib):
    L = hiplib
    conv.set_profiling(True)
    conv.upload_scene(synth.unit_quad())
    for pipe in ("auto", "multipass", "team", "lean"):
        conv.set_pipeline(pipe)
        assert conv.convert(16) == 256
        k = conv.last_kernel_ms()
        print(f"conversion, {pipe} -> {conv.last_pipeline}: {k}")
        assert all(math.isfinite(v) and v >= 0 for v in k.values()), k
        # multi-pass: count + scan and emit; single-pass: the fused kernel (and the second stage where it deferred triangles; a form
        # that was demoted on the way leaves its entry behind too)
        if conv.last_pipeline == "multipass":
            assert k["count"] > 0 and k["emit"] > 0, k
        else:
            assert k["fused"] > 0, k
        # resetting: an unprofiled conversion zeroes the entries, and nothing else moves
        _, _, after = unchanged_by(L, conv, "convert", lambda: conv.convert(16))
        assert all(v == 0.0 for v in after["kernel"]), after["kernel"]
    conv.set_pipeline("auto")
    print("submit + wait, profiled")
    assert conv.convert(16) == 256                                          # (this R has converted cleanly: the next submission is asynchronous)
    conv.submit(16)
    assert conv.wait() == 256
    k = conv.last_kernel_ms()
    assert any(v > 0 for v in k.values()) and all(math.isfinite(v) and v >= 0 for v in k.values()), k
    print("m2s_records_to_world_units")
    assert conv.to_world_units()["previous_R"] == 16
    expect(times(L, conv), "world_units", POS)
    assert conv.to_world_units()["previous_R"] == 1                         # R <= 1: returns before it measures
    expect(times(L, conv), "world_units", POS)
    assert conv.convert(16) == 256
    _, _, after = unchanged_by(L, conv, "world_units", lambda: conv.to_world_units())
    expect(after, "world_units", ZERO)                                      # resetting


def test_mesh_passes_refit_score_bake(conv, hiplib):
    L = hiplib
    conv.set_profiling(True)
    conv.upload_scene(synth.unit_quad())
    assert conv.convert(16) == 256
    pp = frame(conv, QEYE, QAT)
    print("m2s_mesh_depth, triangles deferred to the binned path")
    counts = conv.mesh_depth(pp, download=False)
    assert counts["pairs"] > 0, counts
    t = times(L, conv)
    expect(t, "mesh_depth_stage", POS, POS, POS)
    assert t["mesh_depth"][0] == f32sum(*t["mesh_depth_stage"])
    unchanged_by(L, conv, "mesh_depth", lambda: conv.mesh_depth(pp, download=False))
    print("m2s_mesh_depth, every triangle drawn in place")
    conv.debug_set_mesh_depth_inplace(8192)
    try:
        counts = conv.mesh_depth(pp, download=False)
        assert counts["pairs"] == 0 and counts["drawn"] > 0, counts
        t = times(L, conv)
        expect(t, "mesh_depth_stage", POS, ZERO, ZERO)
        assert t["mesh_depth"][0] == t["mesh_depth_stage"][0]
    finally:
        conv.debug_set_mesh_depth_inplace(-1)
    print("m2s_mesh_depth, a deferred triangle that gives no pairs")
    # the quad's first triangle (0,0) (1,0) (1,1) alone, taken to clip space by (x, y) -> (-6 + 7 y, 1 - 7 x) with w = 1: vertices
    # (-6, 1), (-6, -6), (1, -6).  No guard-band plane |x|, |y| <= 2 w has all three outside, two have some: the triangle goes to the
    # clipper, and it lies beyond x + y = -5, which the band's corner (-2, -2) does not reach: nothing is left to bin
    corner = np.array([[0, -7, 0, 0], [7, 0, 0, 0], [0, 0, 1, 0], [-6, 1, 0, 1]], F)          # (m[c] is column c)
    beside = PrepassParams(view_mat=np.eye(4, dtype=F), proj_mat=np.eye(4, dtype=F), model_mat=corner, renderer_resolution=(W, H),
                           resolution_target=16)
    conv.set_triangle_range(0, 1)
    try:
        conv.upload_scene(synth.unit_quad())
        counts = conv.mesh_depth(beside, download=False)
        print(f"    counts: {counts}")
        assert counts["pairs"] == 0 and counts["drawn"] == 0, counts
        t = times(L, conv)
        expect(t, "mesh_depth_stage", POS, POS, ZERO)
        assert t["mesh_depth"][0] == f32sum(*t["mesh_depth_stage"])
        unchanged_by(L, conv, "mesh_depth without pairs", lambda: conv.mesh_depth(beside, download=False))
    finally:
        conv.set_triangle_range(0, None)
        conv.upload_scene(synth.unit_quad())
    assert conv.convert(16) == 256
    print("m2s_mesh_render")
    conv.mesh_render(pp, download=False)
    t = times(L, conv)
    expect(t, "mesh_render_stage", POS, POS, POS, POS)
    s = t["mesh_render_stage"]
    assert t["mesh_render"][0] == f32sum(f32sum(s[0], s[1]), f32sum(s[2], s[3]))
    unchanged_by(L, conv, "mesh_render", lambda: conv.mesh_render(pp, download=False))
    print("m2s_refit_accumulate, m2s_refit_apply")
    conv.refit_begin()
    assert conv.prepass_sorted(pp, download=False) > 0
    conv.splat(SplatParams((W, H), 0), download=False)
    rp = RefitParams((W, H), 128)
    assert conv.refit_accumulate(rp)["pairs"] > 0
    expect(times(L, conv), "refit_stage", POS, POS, POS)
    unchanged_by(L, conv, "refit_accumulate", lambda: conv.refit_accumulate(rp))
    conv.refit_apply()
    expect(times(L, conv), "refit_apply", POS)
    conv.refit_begin()
    unchanged_by(L, conv, "refit_apply", lambda: conv.refit_apply())
    print("m2s_shadow, m2s_relight, m2s_relight_mesh, m2s_score_frames")
    lp = light(QEYE)
    per_face, _ = conv.shadow(pp, lp, download=False)
    assert sum(per_face) > 0 and conv.last_shadow_counts()["pairs"] > 0
    t = times(L, conv)
    expect(t, "shadow_stage", POS, POS, POS)
    assert t["shadow"][0] == f32sum(*t["shadow_stage"])
    unchanged_by(L, conv, "shadow", lambda: conv.shadow(pp, lp, download=False))
    conv.relight(lp, download=False)
    t = times(L, conv)
    expect(t, "relight", POS)
    expect(t, "shadow_stage", POS, POS, POS)                               # (the relight leaves the shadow pass's times alone)
    unchanged_by(L, conv, "relight", lambda: conv.relight(lp, download=False))
    conv.relight_mesh(lp, download=False)
    expect(times(L, conv), "relight", POS)
    unchanged_by(L, conv, "relight_mesh", lambda: conv.relight_mesh(lp, download=False))
    conv.relight_split(lp, 0.5, download=False)
    expect(times(L, conv), "relight", POS)
    unchanged_by(L, conv, "relight_split", lambda: conv.relight_split(lp, 0.5, download=False))
    print("m2s_shadow_from_quads: stage B alone")
    lists = [conv.download_shadow_quads(f, per_face[f]) for f in range(6)]
    conv.shadow_from_quads(lists, lp, download=False)
    t = times(L, conv)
    expect(t, "shadow_stage", ZERO, POS, POS)
    assert t["shadow"][0] == f32sum(t["shadow_stage"][1], t["shadow_stage"][2])
    unchanged_by(L, conv, "shadow_from_quads", lambda: conv.shadow_from_quads(lists, lp, download=False))
    print("m2s_shadow_from_quads, no quads")
    conv.shadow_from_quads([np.zeros((0, 12), F)] * 6, lp, download=False)
    expect(times(L, conv), "shadow_stage", ZERO, ZERO, ZERO)
    conv.score_frames(ScoreParams((W, H), 2, False, False))
    expect(times(L, conv), "score", POS)
    unchanged_by(L, conv, "score_frames", lambda: conv.score_frames(ScoreParams((W, H), 2, False, False)))
    print("m2s_bake_light")
    bp = BakeParams(n_theta=4, n_phi=8, use_shadows=False)
    conv.bake_light(bp, lp, download=False)
    expect(times(L, conv), "bake", POS)
    unchanged_by(L, conv, "bake_light", lambda: conv.bake_light(bp, lp, download=False))


def test_shadow_degenerate(conv, hiplib, rec257):
    import torch
    L = hiplib
    conv.set_profiling(True)
    conv.upload_records(rec257)
    pp, lp = frame(conv), light()
    per_face, _ = conv.shadow(pp, lp, download=False)
    assert sum(per_face) > 0
    expect(times(L, conv), "shadow_stage", POS, POS, POS)
    print("m2s_shadow, 0 records")
    per_face, _ = conv.shadow(pp, lp, records=torch.empty((0, 24), dtype=torch.float32, device="cuda"), download=False)
    assert sum(per_face) == 0
    t = times(L, conv)
    expect(t, "shadow_stage", ZERO, ZERO, ZERO)
    expect(t, "shadow", ZERO)
    print("m2s_shadow, records none of which reaches a face (all of them lie in front of the light's near plane)")
    far = LightParams(light_position=(1.5, 2.0, 2.5), camera_position=EYE, renderer_resolution=(W, H), shadow_resolution=S,
                      near_plane=1000.0, far_plane=2000.0)
    per_face, _ = conv.shadow(pp, far, download=False)
    assert sum(per_face) == 0, per_face
    t = times(L, conv)
    expect(t, "shadow_stage", POS, ZERO, ZERO)
    assert t["shadow"][0] == t["shadow_stage"][0]


def test_budget_and_merge(conv, hiplib, rec257):
    L = hiplib
    conv.set_profiling(True)
    print("m2s_prune_budget, 257 records")
    conv.upload_records(rec257)
    assert conv.prune_budget(100, "area")["kept"] == 100
    expect(times(L, conv), "budget_stage", POS, POS, POS)
    conv.upload_records(rec257)
    unchanged_by(L, conv, "prune_budget", lambda: conv.prune_budget(100, "area"))
    print("m2s_prune_budget, 0 records")
    conv.upload_records(np.zeros((0, 24), F))
    assert conv.prune_budget(100, "area")["kept"] == 0
    expect(times(L, conv), "budget_stage", ZERO, ZERO, ZERO)
    # always: the merge pass measures with profiling off too
    for prof in (True, False):
        conv.set_profiling(prof)
        print(f"m2s_merge, profiling {prof}")
        conv.upload_records(rec257)
        before = gated(times(L, conv))
        got = conv.merge(3, 4, 0.5)
        assert got["after"] < 257, got
        expect(times(L, conv), "merge_stage", POS, POS, POS)
        conv.upload_records(rec257)
        conv.merge(3, 4, 0.5, dry_run=True)
        expect(times(L, conv), "merge_stage", POS, POS, ZERO)
        conv.upload_records(rec257)
        got = conv.merge(3, 4, 2.0)                                         # (no two unit axes have a dot product of 2: nothing merges)
        assert got["after"] == 257, got
        expect(times(L, conv), "merge_stage", POS, POS, POS)                # (not a dry run: the reduction runs over 257 segments of one)
        conv.upload_records(np.zeros((0, 24), F))
        conv.merge(3, 4, 0.5)
        expect(times(L, conv), "merge_stage", ZERO, ZERO, ZERO)
        assert gated(times(L, conv)) == before
    conv.set_profiling(True)


def test_lod(conv, hiplib, rec257):
    L = hiplib
    conv.set_profiling(True)
    for prof in (True, False):
        conv.set_profiling(prof)
        print(f"m2s_lod_build, profiling {prof}")
        conv.upload_records(rec257)
        built = conv.lod_build((3, 10), 4, 0.5)
        assert built["leaves"] == 257 and built["levels"] >= 2, built
        expect(times(L, conv), "lod_build", POS)
    conv.set_profiling(True)
    cam, f = EYE, focal()
    print("m2s_lod_select")
    assert conv.lod_select(cam, f, 0.0)["selected"] == 257
    expect(times(L, conv), "lod_select_stage", POS, POS, POS)
    unchanged_by(L, conv, "lod_select", lambda: conv.lod_select(cam, f, 0.0))
    print("m2s_lod_select, dry run")
    conv.lod_select(cam, f, 0.0, dry_run=True)
    expect(times(L, conv), "lod_select_stage", POS, ZERO, ZERO)
    print("m2s_lod_select_budget")
    conv.lod_select_budget(cam, f, 100)
    t = times(L, conv)
    expect(t, "lod_budget_stage", POS, POS, POS)
    expect(t, "lod_select_stage", POS, POS, POS)
    s = t["lod_select_stage"]
    assert t["lod_budget_stage"][2] == f32sum(f32sum(s[0], s[1]), s[2])
    unchanged_by(L, conv, "lod_select_budget", lambda: conv.lod_select_budget(cam, f, 100))
    print("m2s_lod_select_budget, dry run")
    conv.lod_select_budget(cam, f, 100, dry_run=True)
    t = times(L, conv)
    expect(t, "lod_select_stage", POS, ZERO, ZERO)
    assert t["lod_budget_stage"][2] == t["lod_select_stage"][0]
    print("m2s_lod_select_frustum, m2s_lod_select_budget_frustum")
    fr = _ld.frustum_of(frame(conv))
    conv.lod_select(cam, f, 0.0, frustum=fr)
    t = times(L, conv)
    expect(t, "lod_frustum", POS)
    expect(t, "lod_select_stage", POS, POS, POS)
    unchanged_by(L, conv, "lod_select_frustum", lambda: conv.lod_select(cam, f, 0.0, frustum=fr))
    conv.lod_select_budget(cam, f, 100, frustum=fr)
    t = times(L, conv)
    expect(t, "lod_frustum", POS)
    expect(t, "lod_budget_stage", POS, POS, POS)
    unchanged_by(L, conv, "lod_select_budget_frustum", lambda: conv.lod_select_budget(cam, f, 100, frustum=fr))
    print("a step of m2s_lod_build that merges nothing leaves the merge pass's times of a dry run")
    conv.upload_records(rec257)
    built = conv.lod_build((3,), 4, 2.0)
    assert built["levels"] == 1 and built["skipped"] == 1, built
    expect(times(L, conv), "merge_stage", POS, POS, ZERO)
    print("a tree of 0 leaves")
    conv.upload_records(np.zeros((0, 24), F))
    assert conv.lod_build((1,))["nodes"] == 0
    expect(times(L, conv), "lod_build", POS)
    assert conv.lod_select(cam, f, 1.0)["selected"] == 0
    expect(times(L, conv), "lod_select_stage", ZERO, ZERO, ZERO)
    expect(times(L, conv), "lod_frustum", POS)                             # (the plain cut does not touch the frustum's time)
    conv.lod_select_budget(cam, f, 5)
    expect(times(L, conv), "lod_budget_stage", ZERO, ZERO, ZERO)
    conv.lod_select(cam, f, 1.0, frustum=fr)
    expect(times(L, conv), "lod_frustum", ZERO)
    conv.lod_release()


def test_compact_export(conv, hiplib, rec257, tmp_path):
    L = hiplib
    path = str(tmp_path / "c.ply")
    for prof in (True, False):                                              # always
        conv.set_profiling(prof)
        print(f"m2s_export_ply_compact, profiling {prof}")
        conv.upload_records(rec257)
        before = gated(times(L, conv))
        assert conv.export_ply_compact(path)["rows"] == 257
        expect(times(L, conv), "compact_stage", POS, POS, POS, POS)
        conv.upload_records(np.zeros((0, 24), F))
        assert conv.export_ply_compact(path)["rows"] == 0
        expect(times(L, conv), "compact_stage", ZERO, ZERO, ZERO, POS)
        assert gated(times(L, conv)) == before
    conv.set_profiling(True)
