"""Measures the level-of-detail tree and its cut on C3's 2.74 M records at R = 1024, 1920 x 1080: m2s_lod_build with the default chain
(nodes per level, time), m2s_lod_select per stage for the preview camera at distance factors 1, 2, 4, 8 and every --tau; beside each
cut the yardstick — m2s_prune over as many records as the tree has nodes (the node pool itself, adopted), keeping as many as the cut
selected: the same compaction, so the difference is what the selection costs — and, with --frames, the frame's pass times and `score`
against the mesh for the cut, for the full records and for merge_to_budget to the cut's count.

    python tools/lod_probe.py [--tau 1,1024] [--factors 1,2,4,8] [--frames] [--reps 5] [--warmup 2] [--out profiles/lod/probe.json]
    python tools/lod_probe.py --world-units [--tau 1,2,4] [--frames] --out profiles/lod/probe_world.json
    python tools/lod_probe.py --world-units --unsigned-axis [--frames] --out profiles/lod/probe_unsigned.json
    python tools/lod_probe.py --budget [--budgets 50000,200000,1000000] [--out profiles/lod/probe_budget.json]
    python tools/lod_probe.py --frustum [--factors 0.25,0.5,1,2] [--tau 1,2,4] [--budgets ...] [--out profiles/lod/probe_frustum.json]
    python tools/lod_probe.py --occlusion [--factors 0.25,0.5,1,2] [--tau 1,2,4] [--budgets ...] [--out profiles/lod/probe_occlusion.json]

--world-units: every conversion is followed by m2s_records_to_world_units, so the tree's edges are world lengths and tau_px counts
screen pixels (default --tau 1,2,4); the result also carries the pass's own time (in place, and out of place from adopted memory) beside
its two yardsticks on the same records: m2s_refit_apply with every record updated, and a device-to-device copy of the records.

--unsigned-axis: the tree with and without M2S_MERGE_UNSIGNED_AXIS, alternating in this one process: for every cut the records are
converted again and the tree is built for one mode, then for the other (the context keeps one tree), so the build is timed
2 x cuts x (warmup + reps) times; per mode the nodes per level, the build's median and its runs one by one, and per cut the counts,
the stages and — with --frames — the frame of the cut beside the frame of the full records, both scored against the mesh.  The
yardsticks of the plain run (m2s_prune, merge_to_budget, the pass's own time) are left out.

--budget: m2s_lod_select_budget on the tree in world units with M2S_MERGE_UNSIGNED_AXIS, per distance factor and budget: the three
stages, the tau_px and the count it returns, and in the same process the yardstick a caller had without it: 31 M2S_LOD_DRY_RUN calls of
m2s_lod_select that build the same key from its top bit down on the host (each a sweep and a round trip of the counts), then the real
cut at the tau found; their sweeps' device time summed, and the whole search on the host's clock beside the budget call's.

--frustum: m2s_lod_select_frustum and m2s_lod_select_budget_frustum on the same tree (world units, M2S_MERGE_UNSIGNED_AXIS), per distance
factor with the preview camera's own matrices and the prepass's guard band: the leaves inside; per --tau the visibility stage and the
three cut stages beside the plain m2s_lod_select at the same tau, the counts of both, and m2s_prepass_sorted (keys with the frustum
test, radix sort, prepass over the survivors) + m2s_splat of the frame drawn from either result; per budget the tau_px, the counts and
the stages of both budget functions.  The yardstick is the plain calls; which of the two runs first alternates between repetitions.

--occlusion: m2s_lod_select_occluded and m2s_lod_select_budget_occluded in the cells of --frustum (the same tree, cameras, taus and
budgets), each beside the frustum call of the same cell, which is the yardstick: the depth image is the context's own, drawn by
m2s_mesh_depth through the cell's camera at 1920 x 1080, whose time is reported apart (it is what the occluded cut costs on top); per
call the leaves inside the frustum, the occluded ones, the tau_px, the selected records, the quads the frame after it draws (its prepass
runs without the depth test), the visibility stage, the stages of the cut and the whole call on the host's clock.

A conversion stores a record's edges in units the viewer divides by the resolutionTarget, and those are the edges the cut's pin reads:
tau_px = 1024 is one SCREEN pixel per texel edge at R = 1024, tau_px = 1 the pin's own unit.  Stage times come from device events, `host_wall`
is the whole call on the host's clock; medians of --reps calls after --warmup."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tau", default="")
    ap.add_argument("--world-units", action="store_true")
    ap.add_argument("--unsigned-axis", action="store_true")
    ap.add_argument("--factors", default=None)
    ap.add_argument("--frames", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget", action="store_true")
    ap.add_argument("--budgets", default="50000,200000,1000000")
    ap.add_argument("--frustum", action="store_true")
    ap.add_argument("--occlusion", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.frustum + a.budget + a.occlusion > 1:
        ap.error("--frustum, --occlusion and --budget are three runs: give one of them")
    a.factors = a.factors or ("0.25,0.5,1,2" if a.frustum or a.occlusion else "1,2,4,8")
    if a.frustum or a.occlusion:
        a.world_units = True
        a.out = a.out or os.path.join(ROOT, "profiles", "lod", "probe_occlusion.json" if a.occlusion else "probe_frustum.json")
    if a.budget:
        a.world_units = True
        a.out = a.out or os.path.join(ROOT, "profiles", "lod", "probe_budget.json")
    a.tau = a.tau or ("1,2,4" if a.world_units else "1,1024")
    import numpy as np
    from mesh2splat_amd import lod, synth
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.score import camera_from_eye, orbit_eye, preview_rule
    R, W, H = 1024, 1920, 1080
    scene = synth.cube_sphere(289, tex_size=2048)
    conv = Converter(0)
    conv.upload_scene(scene)
    conv.set_max_gaussians(0)
    conv.set_profiling(True)
    ctr, dist, near, far = preview_rule(scene)
    light = (ctr[0] + dist, ctr[1] + dist, ctr[2] + dist)

    def median_of(rows):
        return {k: statistics.median(r[k] for r in rows) for k in rows[0]}

    def camera(f):
        return camera_from_eye(orbit_eye(ctr, dist * f, 0, 1), ctr, near, far * f, W, H)

    def frame(cam):
        """one lit frame of the current records and its score against the mesh -> pass times, score"""
        pp, lp = cam.frame_params(conv.resolution, light, 4.0 * dist * dist)
        s = conv.score(pp, lp)
        return ({"prepass": conv.last_prepass_ms, "sort": conv.last_sort_prepass_ms, "splat": conv.last_splat_ms, "shadow": conv.last_shadow_ms,
                 "relight": conv.last_relight_ms}, {"psnr_db": s.psnr, "ssim": s.ssim})

    def convert():
        n = conv.convert(R)
        if a.world_units:
            conv.to_world_units()
        return n

    def pass_times():
        """the pass in place and out of place, m2s_refit_apply with every record updated, a device-to-device copy: medians (ms)"""
        import torch
        n = conv.convert(R)
        out = {"in_place": [], "out_of_place": [], "refit_apply": [], "d2d_copy": []}
        src = torch.empty(n * 24, dtype=torch.float32, device="cuda")
        dst = torch.empty_like(src)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for k in range(a.warmup + a.reps):
            conv.convert(R)
            t = [conv.to_world_units()["ms"]]
            conv.set_records(src.data_ptr(), n, R)
            t.append(conv.to_world_units()["ms"])
            conv.convert(R)
            conv.refit_begin()
            conv.upload_refit(np.zeros((n, 3), np.int64), np.full(n, 1 << 17, np.uint64))
            assert conv.refit_apply(1.0, 1.0)["updated"] == n
            t.append(conv.last_refit_stage_ms()["apply"])
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            torch.cuda.synchronize()
            t.append(ev[0].elapsed_time(ev[1]))
            if k >= a.warmup:
                for key, v in zip(out, t):
                    out[key].append(v)
        return {key: statistics.median(v) for key, v in out.items()}

    def cut_rows(eye, focal, tau, cam):
        rows, counts = [], None
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            got = conv.lod_select(eye, focal, tau, cam.near)
            wall = (time.perf_counter() - t0) * 1e3
            assert counts is None or got == counts                                    # integer sums: the same from run to run
            counts = got
            ms = conv.last_lod_select_stage_ms()
            ms["total"] = ms["sweep"] + ms["scan_ids"] + ms["compact"]
            ms["host_wall"] = wall                                                    # (the whole call on the host's clock, the binding included)
            if k >= a.warmup:
                rows.append(ms)
        return counts, median_of(rows)

    if a.frustum or a.occlusion:
        from mesh2splat_amd.meshdepth import MeshDepthParams
        from mesh2splat_amd.splat import SplatParams
        yard, mine = ("frustum", "occluded") if a.occlusion else ("plain", "frustum")     # the yardstick and the call measured against it
        records = convert()
        build = conv.lod_build(unsigned_axis=True)
        first = build["first"]
        res = {"scene": "c3", "density": R, "size": [W, H], "records": records, "reps": a.reps, "warmup": a.warmup, "world_units": True, "unsigned_axis": True,
               "guard_band": 1.05,
               "build": {"counts": {k: v for k, v in build.items() if k != "first"}, "per_level_nodes": [first[l + 1] - first[l] for l in range(len(first) - 1)],
                         "ms": conv.last_lod_build_ms}, "cells": []}

        def draw(cam):
            """m2s_prepass_sorted + m2s_splat of the current records -> (quads drawn, pass times).  prepass_sorted reports its stages
            through the depth sort's counters: the keys (with the frustum test) over every record handed over, the radix sort, then the
            prepass over the survivors; last_sort_ms spans the three"""
            pp, _ = cam.frame_params(conv.resolution, light, 4.0 * dist * dist)
            drawn = conv.prepass_sorted(pp, download=False)
            st = conv.last_sort_stage_ms
            ms = {"keys": st["keys"], "radix_sort": st["radix_sort"], "prepass": st["gather"], "prepass_sorted": conv.last_sort_ms}
            conv.splat(SplatParams((W, H), 0), download=False)
            ms["splat"] = conv.last_splat_ms
            ms["total"] = ms["prepass_sorted"] + ms["splat"]
            return drawn, ms

        def pair(cam, call, stages, fr, occ=None):
            """warmup + reps of one cut without and with the frustum (--occlusion: with the frustum, without and with the occluder), each
            followed by its frame; which of the two runs first alternates from one repetition to the next
            -> {yard | mine: (result, quads drawn, median stages, median frame passes)}"""
            modes = ((yard, {"frustum": fr}), (mine, {"frustum": fr, "occluder": occ})) if a.occlusion else ((yard, {"frustum": None}), (mine, {"frustum": fr}))
            rows, frames, got, drawn = {yard: [], mine: []}, {yard: [], mine: []}, {}, {}
            for k in range(a.warmup + a.reps):
                for name, kw in (modes if k % 2 == 0 else modes[::-1]):
                    t0 = time.perf_counter()
                    now = call(**kw)
                    call_ms = (time.perf_counter() - t0) * 1e3
                    assert name not in got or now == got[name]                        # integer sums: the same from run to run
                    got[name] = now
                    ms = stages(kw["frustum"])
                    if a.occlusion:
                        ms["call"] = call_ms                                          # (the host's clock: the counts' round trips and the dict included)
                    drawn[name], fm = draw(cam)
                    if k >= a.warmup:
                        rows[name].append(ms)
                        frames[name].append(fm)
            return {name: (got[name], drawn[name], median_of(rows[name]), median_of(frames[name])) for name, _ in modes}

        def select_stages(frustum):
            ms = conv.last_lod_select_stage_ms()
            if frustum:
                ms["visibility"] = conv.last_lod_frustum_ms()
            ms["total"] = sum(ms.values())
            return ms

        def mesh_depth_ms(cam):
            """m2s_mesh_depth through this camera at W x H, warmup + reps times: the image stays the context's -> median ms"""
            rows = []
            for k in range(a.warmup + a.reps):
                conv.mesh_depth(MeshDepthParams(cam.view_mat, cam.proj_mat, np.eye(4, dtype=np.float32), (W, H)), download=False)
                if k >= a.warmup:
                    rows.append(conv.last_mesh_depth_ms)
            return statistics.median(rows)

        def budget_stages(frustum):
            ms = dict(conv.last_lod_budget_stage_ms)
            if frustum:
                ms["visibility"] = conv.last_lod_frustum_ms()
            ms["total"] = sum(ms.values())
            return ms

        for f in [float(v) for v in a.factors.split(",")]:
            cam = camera(f)
            eye, focal = lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H)
            fr = lod.frustum_to_c(np.eye(4, dtype=np.float32), cam.view_mat, cam.proj_mat, 1.05)
            cell = {"factor": f, "cuts": [], "budgets": []}
            occ = None
            if a.occlusion:
                cell["mesh_depth_ms"] = mesh_depth_ms(cam)                            # counted apart: no cut's time holds it
                occ = lod.occluder_of_mesh_depth(conv)
            for tau in [float(v) for v in a.tau.split(",")]:
                row = {"tau_px": tau}
                for name, (got, drawn, stage, fm) in pair(cam, lambda **kw: conv.lod_select(eye, focal, tau, cam.near, **kw), select_stages, fr, occ).items():
                    row[name] = {"counts": got, "quads_drawn": drawn, "select_stage_ms": stage, "frame_pass_ms": fm}
                cell["visible_leaves"] = row[mine]["counts"]["visible_leaves"]
                if a.occlusion:
                    cell["occluded_leaves"] = row[mine]["counts"]["occluded_leaves"]
                cell["cuts"].append(row)
            for budget in [int(v) for v in a.budgets.split(",")]:
                row = {"budget": budget}
                for name, (got, drawn, stage, fm) in pair(cam, lambda **kw: conv.lod_select_budget(eye, focal, budget, near=cam.near, **kw),
                                                          budget_stages, fr, occ).items():
                    row[name] = {"result": got, "quads_drawn": drawn, "budget_stage_ms": stage, "frame_pass_ms": fm}
                cell["budgets"].append(row)
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
        conv.close()
        return
    if a.budget:
        records = convert()
        build = conv.lod_build(unsigned_axis=True)
        first = build["first"]
        last = first[-1] - first[-2]
        res = {"scene": "c3", "density": R, "size": [W, H], "records": records, "reps": a.reps, "warmup": a.warmup, "world_units": True, "unsigned_axis": True,
               "build": {"counts": {k: v for k, v in build.items() if k != "first"}, "per_level_nodes": [first[l + 1] - first[l] for l in range(len(first) - 1)],
                         "ms": conv.last_lod_build_ms}, "cells": []}

        def host_bisection(eye, focal, cam, n_eff):
            """the smallest key whose cut holds at most n_eff records, by 31 dry runs -> (key, their sweeps' ms summed)"""
            key, sweep = 0, 0.0
            for bit in range(30, -1, -1):
                c = key | (1 << bit)
                tau = float(np.array([c - 1], np.uint32).view(np.float32)[0])
                if not np.isfinite(tau):
                    continue                                                          # (no finite tau_px there: no cut refines at such a key)
                got = conv.lod_select(eye, focal, tau, cam.near, dry_run=True)
                sweep += conv.last_lod_select_stage_ms()["sweep"]
                if got["selected"] > n_eff:
                    key = c
            return key, sweep

        for f in [float(v) for v in a.factors.split(",")]:
            cam = camera(f)
            eye, focal = lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H)
            for budget in [int(v) for v in a.budgets.split(",")]:
                rows, yard, got = [], [], None
                for k in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    now = conv.lod_select_budget(eye, focal, budget, near=cam.near)
                    wall = (time.perf_counter() - t0) * 1e3
                    assert got is None or now == got                                  # integer sums: the same from run to run
                    got = now
                    ms = dict(conv.last_lod_budget_stage_ms, host_wall=wall)
                    ms["search"] = ms["thresholds"] + ms["select"]
                    ms["total"] = ms["search"] + ms["cut"]
                    t0 = time.perf_counter()
                    key, sweeps = host_bisection(eye, focal, cam, max(budget, last))
                    tau = float(np.array([key], np.uint32).view(np.float32)[0])
                    final = conv.lod_select(eye, focal, tau, cam.near)
                    wall = (time.perf_counter() - t0) * 1e3
                    cut = conv.last_lod_select_stage_ms()
                    assert tau == got["tau_px"] and final == {k: got[k] for k in final}     # the two searches agree
                    if k >= a.warmup:
                        rows.append(ms)
                        yard.append({"search": sweeps, "cut": cut["sweep"] + cut["scan_ids"] + cut["compact"], "host_wall": wall})
                cell = {"factor": f, "budget": budget, "result": got, "budget_stage_ms": median_of(rows), "host_bisection_31_dry_runs_ms": median_of(yard)}
                res["cells"].append(cell)
                print(json.dumps(cell), flush=True)
        print(json.dumps(res))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        conv.close()
        return
    if a.unsigned_axis:
        records = convert()
        names = {False: "signed", True: "unsigned"}
        builds, build_ms = {False: None, True: None}, {False: [], True: []}
        res = {"scene": "c3", "density": R, "size": [W, H], "records": records, "reps": a.reps, "warmup": a.warmup, "world_units": a.world_units, "cuts": []}
        for tau in [float(v) for v in a.tau.split(",")]:
            for f in [float(v) for v in a.factors.split(",")]:
                cam = camera(f)
                eye, focal = lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H)
                row = {"tau_px": tau, "factor": f}
                for m in (False, True):
                    for k in range(a.warmup + a.reps):
                        convert()
                        got = conv.lod_build(unsigned_axis=m)
                        assert builds[m] is None or got == builds[m]
                        builds[m] = got
                        if k >= a.warmup:
                            build_ms[m].append(conv.last_lod_build_ms)
                    counts, stage = cut_rows(eye, focal, tau, cam)
                    row[names[m]] = {"counts": counts, "select_stage_ms": stage}
                    if a.frames:
                        row[names[m]]["frame_cut"] = dict(zip(("pass_ms", "score"), frame(cam)))
                if a.frames:
                    convert()
                    row["frame_full"] = dict(zip(("pass_ms", "score"), frame(cam)))
                res["cuts"].append(row)
                print(json.dumps(row), flush=True)
        for m in (False, True):
            first = builds[m]["first"]
            res["build_" + names[m]] = {"counts": {k: v for k, v in builds[m].items() if k != "first"},
                                        "per_level_nodes": [first[l + 1] - first[l] for l in range(len(first) - 1)],
                                        "ms": statistics.median(build_ms[m]), "ms_min": min(build_ms[m]), "ms_max": max(build_ms[m]), "runs": len(build_ms[m])}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        conv.close()
        return
    records = conv.convert(R)
    build_ms, build = [], None
    for k in range(a.warmup + a.reps):
        convert()
        got = conv.lod_build()
        assert build is None or got == build
        build = got
        if k >= a.warmup:
            build_ms.append(conv.last_lod_build_ms)
    first = build["first"]
    res = {"scene": "c3", "density": R, "size": [W, H], "records": records, "reps": a.reps, "warmup": a.warmup, "world_units": a.world_units,
           "build": {"counts": {k: v for k, v in build.items() if k != "first"}, "per_level_nodes": [first[l + 1] - first[l] for l in range(len(first) - 1)],
                     "ms": statistics.median(build_ms)}, "cuts": []}
    if a.world_units:
        res["pass_ms"] = pass_times()
        print(json.dumps({"pass_ms": res["pass_ms"]}), flush=True)
    nodes = build["nodes"]
    unit_R = 1 if a.world_units else R                                              # the resolutionTarget of the tree's leaves
    for tau in [float(v) for v in a.tau.split(",")]:
        for f in [float(v) for v in a.factors.split(",")]:
            cam = camera(f)
            eye, focal = lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H)
            counts, stage = cut_rows(eye, focal, tau, cam)
            row = {"tau_px": tau, "factor": f, "counts": counts, "select_stage_ms": stage}
            ids = conv.download_lod_nodes()
            if a.frames:
                row["frame_cut"] = dict(zip(("pass_ms", "score"), frame(cam)))
            # the yardstick: m2s_prune over the node pool, keeping the same nodes
            keep = np.zeros(nodes, np.uint32)
            keep[ids] = 1
            prune_ms = []
            for k in range(a.warmup + a.reps):
                conv.set_records(conv.device_lod(0), nodes, unit_R)
                conv.contrib_begin()
                conv.upload_contrib(np.ones(nodes, np.float32), keep)
                assert conv.prune(0.5, 1)["kept"] == counts["selected"]
                if k >= a.warmup:
                    prune_ms.append(conv.last_prune_ms)
            row["prune_same_counts_ms"] = statistics.median(prune_ms)
            if a.frames:
                convert()
                row["frame_full"] = dict(zip(("pass_ms", "score"), frame(cam)))
                mb = conv.merge_to_budget(max(counts["selected"], 1))
                row["frame_merge_to_budget"] = dict(zip(("pass_ms", "score"), frame(cam)), level=mb["level"], met=mb["met"], after=mb["after"])
            res["cuts"].append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    conv.close()


if __name__ == "__main__":
    main()
