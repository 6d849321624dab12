"""Measures m2s_prune_budget on C3's 2.74 M records: convert -> m2s_prepass_sorted -> m2s_contrib_accumulate (one 1920 x 1080 view) ->
m2s_prune_budget to --budget records, VIEWS and AREA, profiling on; against m2s_prune (the yardstick: the existing compaction, in the same
process on the same records) with min_weight = the float whose bits are T, and with min_weight at the wmax that keeps as many records as
the budget.

    python tools/budget_probe.py [--size 1920x1080] [--budget 1000000] [--reps 5] [--warmup 2] [--out profiles/budget/probe.json]

Stage times come from device events (m2s_last_budget_stage_ms, m2s_last_prune_ms): medians of --reps calls after --warmup; between calls
the state is put back by converting and accumulating again, outside the timed span."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--budget", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    import numpy as np
    import camera
    from mesh2splat_amd import synth
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.prepass import PrepassParams
    from mesh2splat_amd.splat import SplatParams
    R = 1024
    conv = Converter(0)
    conv.upload_scene(synth.cube_sphere(289, tex_size=2048))
    conv.set_max_gaussians(0)
    pp = PrepassParams(view_mat=camera.look_at((1.6, 1.1, 2.3), (0.1, 0.0, -0.1)), proj_mat=camera.perspective(45.0, W / H, 0.01, 100.0),
                       renderer_resolution=(W, H), resolution_target=R, render_mode=0)
    sp = SplatParams((W, H), 0)
    conv.set_profiling(True)

    def restore(views: bool):
        n = conv.convert(R)
        if views:
            conv.contrib_begin()
            conv.prepass_sorted(pp, download=False)
            conv.contrib_accumulate(sp, 1.0 / 255.0)
        return n

    def median_of(rows):
        return {k: statistics.median(r[k] for r in rows) for k in rows[0]}

    records = restore(True)
    wmax, npix = conv.download_contrib()
    res = {"scene": "c3", "density": R, "size": [W, H], "records": records, "budget": a.budget, "reps": a.reps, "warmup": a.warmup,
           "seen_records": int((wmax > 0).sum())}
    for importance in ("views", "area"):
        rows, counts = [], None
        for k in range(a.warmup + a.reps):
            restore(importance == "views")
            got = conv.prune_budget(a.budget, importance, -1.0, 0)
            assert counts is None or got == counts, (got, counts)          # integer arithmetic: the same from run to run
            counts = got
            ms = conv.last_budget_stage_ms()
            ms["total"] = ms["select"] + ms["flags_scans"] + ms["compact"]
            if k >= a.warmup:
                rows.append(ms)
        res[importance] = {"counts": counts, "stage_ms": median_of(rows)}
    # the yardstick: m2s_prune on the same records and accumulators
    T = np.array([res["views"]["counts"]["threshold_key"]], np.uint32).view(np.float32)[0]
    as_many = float(np.sort(wmax)[max(0, wmax.size - a.budget - 1)]) if wmax.size > a.budget else -1.0
    for name, tau in (("prune_at_T", float(T)), ("prune_as_many", as_many)):
        times, counts = [], None
        for k in range(a.warmup + a.reps):
            restore(True)
            counts = conv.prune(tau, 0)
            if k >= a.warmup:
                times.append(conv.last_prune_ms)
        res[name] = {"min_weight": tau, "counts": counts, "ms": statistics.median(times)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    conv.close()


if __name__ == "__main__":
    main()
