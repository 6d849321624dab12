"""-m gpu: what every way of replacing the context's current records does to everything whose validity hangs on them (the table of
mesh2splat_amd/csrc/m2s_recstate.h, seen through the Python wrappers and the public getters).

Every case first establishes all the dependents at once on 16 records (a conversion of synth.unit_quad() at R = 8, 64 records, merged
once by m2s_lod_build): the depth sort, sorted quads with sources, the contribution and the refit accumulators, a merge map or the node
indices of a cut, a baked SH plane with tap counts, the position plane.  Then it replaces the records by one route and records every
observer.  EXPECT holds what the entry points did before the state moved into one type, read off their code; it is a literal table and
is not computed from the library under test.  The two flavours differ in what cannot exist at once:
    "map": the merge map; sorted quads from m2s_prepass_sorted (compacting path: the sources survive the depth sort); no prepass quads
    "ids": the node indices of a cut; prepass quads, sorted by m2s_sort_prepass, sources from m2s_upload_quad_sources
Cells: K kept as established, D dropped (0 / NULL), S set by the route itself; a number is the value itself; (status, message) pairs
are what the call returns and m2s_last_error says, OK = (0, "")."""
import ctypes as C

import numpy as np
import pytest

import camera
from mesh2splat_amd import lod as _ld, refit as _rf, splat as _sp, synth
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prepass import PrepassParams

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, STATE = 1, 7
W, H = 160, 90
EYE, AT = (0.5, 0.5, 2.0), (0.5, 0.5, 0.0)
FOCAL = 108.6

IN_FLIGHT = "conversions are still in flight: m2s_convert_wait first"
STALE = ("the records of the conversion last waited for have been overwritten by a later submission at another R "
         "(wait for it, or submit into your own buffers)")
NONE = "no conversion has run and no records were uploaded"
OK = (0, "")
C_CHANGED = (INVALID, "the records changed since m2s_contrib_begin")
C_NO_BEGIN = (INVALID, "no m2s_contrib_begin")
R_CHANGED = (INVALID, "the records changed since m2s_refit_begin")
R_NO_BEGIN = (INVALID, "no m2s_refit_begin")
C_NO_ACC = (STATE, "no accumulators of the current records (m2s_contrib_begin)")
R_NO_ACC = (STATE, "no accumulators of the current records (m2s_refit_begin)")
NO_SH = (STATE, "no baked coefficients for this many records (run m2s_bake_light on them)")
NO_COUNTS = (STATE, "the last m2s_bake_light kept no shadow counts (want_shadow_counts)")
K, D, S, M = "kept", "dropped", "set", "as many as before"

COLUMNS = ("stored", "positions", "sorted", "R", "quads", "sorted_quads", "sources", "merge_map", "lod_nodes", "sh",
           "contrib_accumulate", "refit_accumulate", "download_contrib", "download_refit", "compact_baked", "bake_counts")
# a conversion, an awaited slot and a replaced scene touch nothing but the records themselves: what hangs on an epoch goes, the counts
# (sorted records, quads) and the baked plane stay; uploads and adoptions also zero the three counts; the passes that rewrite the
# records into the pool zero them, drop the sources and the contribution accumulators, and differ in what else they drop
EXPECT = {
    #                  stored positions sorted R  quads sorted_q sources map lod sh  contrib_acc refit_acc  dl_contrib dl_refit  compact    counts
    "convert":        (256,   D,        K,     16, K,   K,       D,      D,  D,  K,  C_CHANGED,  R_CHANGED, C_NO_ACC,  R_NO_ACC, NO_SH,     OK),
    "convert_into":   (256,   D,        K,     16, K,   K,       D,      D,  D,  K,  C_CHANGED,  R_CHANGED, C_NO_ACC,  R_NO_ACC, NO_SH,     OK),
    "submit_wait":    (64,    D,        K,     8,  K,   K,       D,      D,  D,  K,  C_CHANGED,  R_CHANGED, C_NO_ACC,  R_NO_ACC, NO_SH,     OK),
    # two submissions at different R into the context's buffer: the first wait finds its records overwritten, and one is in flight
    "stale_first":    (64,    D,        K,     8,  K,   K,       D,      D,  D,  K,  C_CHANGED,  R_CHANGED, C_NO_ACC,  R_NO_ACC, (STATE, IN_FLIGHT), OK),
    "stale_second":   (256,   D,        K,     16, K,   K,       D,      D,  D,  K,  C_CHANGED,  R_CHANGED, C_NO_ACC,  R_NO_ACC, NO_SH,     OK),
    # (as many records as the plane holds: the plane of the OLD records is taken for theirs)
    "upload_records": (M,     D,        D,     0,  D,   D,       D,      D,  D,  K,  C_CHANGED,  R_CHANGED, C_NO_ACC,  R_NO_ACC, OK,        OK),
    "set_records":    (M,     D,        D,     5,  D,   D,       D,      D,  D,  K,  C_CHANGED,  R_CHANGED, C_NO_ACC,  R_NO_ACC, OK,        OK),
    "upload_scene":   (0,     D,        K,     8,  K,   K,       D,      D,  D,  K,  C_CHANGED,  R_CHANGED, C_NO_ACC,  R_NO_ACC, (STATE, NONE), OK),
    # (the plane is compacted with the records and stays theirs; its tap counts are not)
    "prune":          (M,     D,        D,     8,  D,   D,       D,      D,  D,  K,  C_NO_BEGIN, R_CHANGED, C_NO_ACC,  R_NO_ACC, OK,        NO_COUNTS),
    "prune_budget":   (5,     D,        D,     8,  D,   D,       D,      D,  D,  K,  C_NO_BEGIN, R_CHANGED, C_NO_ACC,  R_NO_ACC, OK,        NO_COUNTS),
    "refit_apply":    (M,     D,        D,     8,  D,   D,       D,      D,  D,  D,  C_NO_BEGIN, R_NO_BEGIN, C_NO_ACC, R_NO_ACC, NO_SH,     NO_COUNTS),
    "merge":          (None,  D,        D,     8,  D,   D,       D,      S,  D,  D,  C_NO_BEGIN, R_NO_BEGIN, C_NO_ACC, R_NO_ACC, NO_SH,     NO_COUNTS),
    # (the cuts drop the plane and keep the refit accumulators' flag: "changed", not "no begin")
    "lod_select":     (64,    D,        D,     8,  D,   D,       D,      D,  S,  D,  C_NO_BEGIN, R_CHANGED, C_NO_ACC,  R_NO_ACC, NO_SH,     NO_COUNTS),
    "lod_budget":     (M,     D,        D,     8,  D,   D,       D,      D,  S,  D,  C_NO_BEGIN, R_CHANGED, C_NO_ACC,  R_NO_ACC, NO_SH,     NO_COUNTS),
    "lod_frustum":    (64,    D,        D,     8,  D,   D,       D,      D,  S,  D,  C_NO_BEGIN, R_CHANGED, C_NO_ACC,  R_NO_ACC, NO_SH,     NO_COUNTS),
    "world_units":    (M,     D,        D,     1,  D,   D,       D,      D,  D,  D,  C_NO_BEGIN, R_NO_BEGIN, C_NO_ACC, R_NO_ACC, NO_SH,     NO_COUNTS),
}
assert all(len(row) == len(COLUMNS) for row in EXPECT.values())


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def owner(hiplib):
    c = Converter(0)
    yield c
    c.close()


def frame(conv, depth_test=False):
    return PrepassParams(view_mat=camera.look_at(EYE, AT), proj_mat=camera.perspective(45.0, W / H, 0.01, 100.0), renderer_resolution=(W, H),
                         resolution_target=max(conv.resolution, 1), perform_mesh_depth_test=depth_test,
                         mesh_depth=np.ones((H, W), F) if depth_test else None)


def said(L, conv, status):
    return (int(status), L.m2s_last_error(conv._h).decode() if status else "")


def observe(L, conv, tmp_path):
    h = conv._h
    out = {"stored": conv.num_stored, "positions": bool(L.m2s_positions_ready(h)), "sorted": int(L.m2s_num_sorted(h)),
           "R": int(L.m2s_last_resolution(h)), "quads": bool(L.m2s_device_quads(h)), "sorted_quads": bool(L.m2s_device_sorted_quads(h)),
           "sources": bool(L.m2s_device_sorted_sources(h)), "merge_map": bool(L.m2s_device_merge_map(h)),
           "lod_nodes": bool(L.m2s_device_lod_nodes(h)), "sh": bool(L.m2s_device_sh(h))}
    sp = _sp.to_c(_sp.SplatParams((W, H), 0))
    out["contrib_accumulate"] = said(L, conv, L.m2s_contrib_accumulate(h, C.byref(sp), C.c_float(1.0 / 255.0)))
    rp = _rf.to_c(_rf.RefitParams((W, H), 128))
    out["refit_accumulate"] = said(L, conv, L.m2s_refit_accumulate(h, C.byref(rp), None, None, None))
    n = max(conv.num_stored, 1)
    w, k = np.empty(n, F), np.empty(n, np.uint32)
    out["download_contrib"] = said(L, conv, L.m2s_download_contrib(h, w.ctypes.data, k.ctypes.data, n))
    num, den = np.empty((n, 3), np.int64), np.empty(n, np.uint64)
    out["download_refit"] = said(L, conv, L.m2s_download_refit(h, num.ctypes.data, den.ctypes.data, n))
    counts = (C.c_uint64 * 3)()
    out["compact_baked"] = said(L, conv, L.m2s_export_ply_compact(h, str(tmp_path / "c.ply").encode(), C.c_float(0.65), 1, counts))
    taps = np.empty(4096, np.uint8)
    out["bake_counts"] = said(L, conv, L.m2s_download_bake_shadow_counts(h, taps.ctypes.data, taps.size))
    return out


def establish(L, conv, flavour, tmp_path):
    """-> what observe() sees once every dependent exists"""
    conv.set_triangle_range(0, None)
    conv.upload_scene(synth.unit_quad())
    assert conv.convert(8) == 64
    built = conv.lod_build((8,), 4, 0.5, unsigned_axis=True)                # the tree for the cuts; its one step leaves a merge map
    assert built["levels"] == 2 and 1 <= conv.num_stored < 64, built
    if flavour == "ids":
        cut = conv.lod_select(EYE, FOCAL, 1e9)                             # the coarsest level again, now with node indices
        assert cut["selected"] == built["nodes"] - 64
    m = conv.num_stored
    conv.bake_light(BakeParams(n_theta=4, n_phi=8, use_shadows=False, want_shadow_counts=True), LightParams(light_position=(1.5, 2.0, 2.5)),
                    download=False)
    conv.contrib_begin()
    conv.refit_begin()
    if flavour == "map":
        assert conv.prepass_sorted(frame(conv, depth_test=True), download=False) > 0
    else:
        vis = conv.prepass(frame(conv), download=False)
        assert vis > 0 and conv.sort_prepass(download=False) == vis
        conv.upload_quad_sources(np.zeros(vis, np.uint32))
    assert conv.sort_by_depth(camera.look_at(EYE, AT), download=False) == m
    before = observe(L, conv, tmp_path)
    ids = flavour == "ids"
    assert before == {"stored": m, "positions": True, "sorted": m, "R": 8, "quads": ids, "sorted_quads": True, "sources": True,
                      "merge_map": not ids, "lod_nodes": ids, "sh": True, "contrib_accumulate": before["contrib_accumulate"],
                      "refit_accumulate": before["refit_accumulate"], "download_contrib": OK, "download_refit": OK, "compact_baked": OK,
                      "bake_counts": OK}, before
    # (the two accumulate calls get past the checks of the state: the contribution pass runs, the refit stops at the missing target)
    assert before["contrib_accumulate"] == OK and before["refit_accumulate"][1].startswith("no mesh G-buffer"), before
    return before


def check(route, before, after):
    want = dict(zip(COLUMNS, EXPECT[route]))
    print(route, after)
    for col, cell in want.items():
        if cell is None:
            continue
        got = after[col]
        if cell == M:
            cell = before["stored"]
        elif cell == K:
            cell = before[col]
        elif cell == D:
            cell = type(before[col])(0)
        elif cell == S:
            cell = True
        assert got == cell, (route, col, got, cell)


def replace(L, conv, owner, route):
    """one way of replacing the records; a generator: each next() is one replacement to observe, named by what it yields"""
    if route == "convert":
        assert conv.convert(16) == 256
    elif route == "convert_into":
        import torch
        buf = torch.empty((256, 24), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert conv.convert_into(16, buf.data_ptr(), 256) == 256
        yield route
        conv.upload_records(np.zeros((1, 24), F))                           # (the tensor goes: nothing of the context points at it)
        return
    elif route == "submit_wait":
        conv.submit(8)
        assert conv.wait() == 64
    elif route == "stale":
        conv.submit(8)
        conv.submit(16)
        assert conv.wait() == 64
        yield "stale_first"
        # the refused states an entry point can be in here: one in flight (the check every record-consuming pass makes first) and,
        # for the one consumer without that check, the overwritten records
        assert said(L, conv, L.m2s_contrib_begin(conv._h)) == (STATE, IN_FLIGHT)
        m2v = np.ascontiguousarray(camera.look_at(EYE, AT), F).reshape(16)
        assert said(L, conv, L.m2s_sort_by_depth(conv._h, m2v.ctypes.data_as(C.POINTER(C.c_float)), None)) == (STATE, STALE)
        assert conv.wait() == 256
        yield "stale_second"
        return
    elif route == "upload_records":
        conv.upload_records(conv.download())
    elif route == "set_records":
        owner.upload_records(conv.download())
        conv.set_records(owner.device_records, owner.num_stored, 5)
    elif route == "upload_scene":
        conv.upload_scene(synth.unit_quad())
    elif route == "prune":
        conv.prune(-1.0, 0)
    elif route == "prune_budget":
        conv.prune_budget(5, "area")
    elif route == "refit_apply":
        conv.refit_apply()
    elif route == "merge":
        conv.merge(9, 4, 0.5, unsigned_axis=True)
    elif route == "lod_select":
        conv.lod_select(EYE, FOCAL, 0.0)                                    # tau_px = 0: every leaf
    elif route == "lod_budget":
        conv.lod_select_budget(EYE, FOCAL, 20)
    elif route == "lod_frustum":
        conv.lod_select(EYE, FOCAL, 0.0, frustum=_ld.frustum_of(frame(conv)))
    elif route == "world_units":
        assert conv.to_world_units()["previous_R"] == 8
    else:
        raise AssertionError(route)
    yield route


ROUTES = ("convert", "convert_into", "submit_wait", "stale", "upload_records", "set_records", "upload_scene", "prune", "prune_budget",
          "refit_apply", "merge", "lod_select", "lod_budget", "lod_frustum", "world_units")


@pytest.mark.parametrize("flavour", ("map", "ids"))
@pytest.mark.parametrize("route", ROUTES)
def test_route(conv, owner, hiplib, tmp_path, route, flavour):
    before = establish(hiplib, conv, flavour, tmp_path)
    for row in replace(hiplib, conv, owner, route):
        check(row, before, observe(hiplib, conv, tmp_path))


def test_refused_states(hiplib, tmp_path):
    """m2s_contrib_begin, one of the entry points that open with the shared check, in the states it refuses: no records, one conversion
    in flight; and an empty shard, which is a conversion like any other.  (Overwritten records exist only while a later submission
    is in flight, so that check is never reached behind the in-flight one: test_route's "stale" case pins both messages.)"""
    L = hiplib
    c = Converter(0)
    try:
        assert said(L, c, L.m2s_contrib_begin(c._h)) == (STATE, NONE)
        assert said(L, c, L.m2s_refit_begin(c._h)) == (STATE, NONE)
        counts = (C.c_uint64 * 3)()
        assert said(L, c, L.m2s_export_ply_compact(c._h, str(tmp_path / "n.ply").encode(), C.c_float(0.65), 0, counts)) == (STATE, NONE)
        c.upload_scene(synth.unit_quad())
        assert said(L, c, L.m2s_contrib_begin(c._h)) == (STATE, NONE)       # a scene is not records
        c.submit(8)
        for fn in (L.m2s_contrib_begin, L.m2s_refit_begin):
            assert said(L, c, fn(c._h)) == (STATE, IN_FLIGHT)
        assert said(L, c, L.m2s_records_to_world_units(c._h, None)) == (STATE, IN_FLIGHT)
        assert c.wait() == 64
        assert said(L, c, L.m2s_contrib_begin(c._h)) == OK
        # the empty shard: zero records at R = 8 behind a pointer, and every dependent can be taken of them
        c.set_triangle_range(0, 0)
        c.upload_scene(synth.unit_quad())
        assert said(L, c, L.m2s_contrib_begin(c._h)) == (STATE, NONE)
        assert c.convert(8) == 0 and c.num_stored == 0 and c.device_records and c.resolution == 8
        assert said(L, c, L.m2s_contrib_begin(c._h)) == OK and said(L, c, L.m2s_refit_begin(c._h)) == OK
        assert L.m2s_device_contrib(c._h, 0) and L.m2s_device_refit(c._h, 0) and not L.m2s_positions_ready(c._h)
        assert c.convert(8) == 0                                            # the same pointer, another epoch
        sp = _sp.to_c(_sp.SplatParams((W, H), 0))
        assert said(L, c, L.m2s_contrib_accumulate(c._h, C.byref(sp), C.c_float(1.0 / 255.0))) == C_CHANGED
        assert not L.m2s_device_contrib(c._h, 0) and not L.m2s_device_refit(c._h, 0)
    finally:
        c.close()
