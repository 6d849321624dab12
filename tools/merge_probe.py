"""Measures m2s_merge on C3's 2.74 M records: convert -> merge at --level (or, with --to N, at the level merge_to_budget finds), the three
stages; beside it, in the same process on the same records, the two things the pass is made of and competes with: m2s_prune_budget AREA
to the count the merge reached, and the box + keys and sort stages of the compact export.

    python tools/merge_probe.py [--level 2 | --to 700000] [--group 4] [--dot 0.5] [--reps 5] [--warmup 2] [--out profiles/merge/probe.json]
    python tools/merge_probe.py --world-units [...] --out profiles/merge/probe_world.json
    python tools/merge_probe.py --world-units --unsigned-axis [...] --out profiles/merge/probe_unsigned.json

--world-units: every conversion is followed by m2s_records_to_world_units, so the merge reads the edges the viewer draws; the result
carries the median longer edge before and after the merge either way (a 2 x 2 block of texels should double it).

--unsigned-axis: the merge with and without M2S_MERGE_UNSIGNED_AXIS, alternating call by call in this one process (the comparison that
tells the two apart is the one within a process: same clocks, same allocations); counts per level and the stages of both, and nothing of
the competitors.  Every result also lists the timed calls' totals one by one ("total_ms_runs"): their spread is the run-to-run noise a
difference between two builds has to be read against.

Stage times come from device events (m2s_last_merge_stage_ms, m2s_last_budget_stage_ms, m2s_last_compact_stage_ms): medians of --reps
calls after --warmup; between calls the records are put back by converting again, outside the timed span."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--to", type=int, default=0)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--dot", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--world-units", action="store_true")
    ap.add_argument("--unsigned-axis", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    from mesh2splat_amd import synth
    from mesh2splat_amd.converter import Converter
    R = 1024
    conv = Converter(0)
    conv.upload_scene(synth.cube_sphere(289, tex_size=2048))
    conv.set_max_gaussians(0)
    conv.set_profiling(True)

    def convert():
        n = conv.convert(R)
        if a.world_units:
            conv.to_world_units()
        return n

    def median_edge():
        rec = conv.download()
        return float(np.median(np.fmax(np.abs(rec[:, 8]), np.abs(rec[:, 9]))))

    def median_of(rows):
        return {k: statistics.median(r[k] for r in rows) for k in rows[0]}

    def merge_rows(modes):
        """the timed merges at `level`, the modes alternating -> per mode: counts, stage medians, the totals one by one"""
        rows, dry_rows, counts = {m: [] for m in modes}, {m: [] for m in modes}, {m: None for m in modes}
        for k in range(a.warmup + a.reps):
            for m in modes:
                convert()
                conv.merge(level, a.group, a.dot, dry_run=True, unsigned_axis=m)
                dry = conv.last_merge_stage_ms()
                got = conv.merge(level, a.group, a.dot, unsigned_axis=m)
                assert counts[m] is None or got == counts[m], (got, counts[m])    # integer logic and exact fp32: the same from run to run
                counts[m] = got
                ms = conv.last_merge_stage_ms()
                ms["total"] = ms["keys_sort"] + ms["heads_scans"] + ms["reduce"]
                if k >= a.warmup:
                    rows[m].append(ms)
                    dry_rows[m].append({"keys_sort": dry["keys_sort"], "heads_scans": dry["heads_scans"]})
        return {m: {"counts": counts[m], "stage_ms": median_of(rows[m]), "dry_run_stage_ms": median_of(dry_rows[m]),
                    "total_ms_runs": [r["total"] for r in rows[m]]} for m in modes}

    records = convert()
    edge_before = median_edge()
    if a.unsigned_axis:
        level = a.level
        res = {"scene": "c3", "density": R, "records": records, "level": level, "max_group": a.group, "min_axis_dot": a.dot, "reps": a.reps,
               "warmup": a.warmup, "world_units": a.world_units, "median_longer_edge_before": edge_before}
        got = merge_rows((False, True))
        for m, name in ((False, "signed"), (True, "unsigned")):
            convert()
            got[m]["after_per_level"] = {lv: conv.merge_count(lv, a.group, a.dot, unsigned_axis=m) for lv in range(11)}
            conv.merge(level, a.group, a.dot, unsigned_axis=m)
            got[m]["median_longer_edge_after"] = median_edge()
            res[name] = got[m]
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        conv.close()
        return
    per_level = {lv: conv.merge_count(lv, a.group, a.dot) for lv in range(11)}
    level = a.level
    if a.to:
        level = conv.merge_to_budget(a.to, a.group, a.dot)["level"]
    res = {"scene": "c3", "density": R, "records": records, "level": level, "max_group": a.group, "min_axis_dot": a.dot, "reps": a.reps,
           "warmup": a.warmup, "world_units": a.world_units, "after_per_level": per_level}
    res["merge"] = merge_rows((False,))[False]
    counts = res["merge"]["counts"]
    res["merge"]["median_longer_edge"] = {"before": edge_before, "after": median_edge()}
    # what it competes with: dropping to the same count
    rows, bcounts = [], None
    for k in range(a.warmup + a.reps):
        convert()
        bcounts = conv.prune_budget(counts["after"], "area")
        ms = conv.last_budget_stage_ms()
        ms["total"] = ms["select"] + ms["flags_scans"] + ms["compact"]
        if k >= a.warmup:
            rows.append(ms)
    res["budget_area"] = {"counts": bcounts, "stage_ms": median_of(rows)}
    # what it is made of: the compact export's order
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        convert()
        for k in range(a.warmup + a.reps):
            ms = conv.export_ply_compact(os.path.join(tmp, "probe.ply"))["stage_ms"]
            if k >= a.warmup:
                rows.append({"box_keys": ms["box_keys"], "sort": ms["sort"]})
    res["compact_export"] = {"stage_ms": median_of(rows)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    conv.close()


if __name__ == "__main__":
    main()
