"""Measures the merge pass under M2S_MERGE_MODEL_GAUSSIAN (m2s_set_merge_model) beside the footprint model, on C3's 2.74 M records at
R = 1024 moved to world units, in one process:

  time    a level-2 m2s_merge and a default-chain m2s_lod_build under both models (sigma = --sigma for the Gaussian one), the models
          alternating.  The reduction is stage [2] of m2s_last_merge_stage_ms (the reduction kernel and the copy of the parents into
          the pool); the Gaussian model's is reported as a ratio to the footprint's, k_merge_reduce, on the same records.
  score   under each model the records are merged to at most half their count (merge_to_budget) and scored against the mesh render
          through --views orbit cameras (Converter.score_views).  The footprint model is what a conversion's records are; the pin's
          own note predicts that reading them as Gaussians shrinks the parents.  Whatever comes out is written down.

    python tools/merge_gauss_probe.py [--sigma 0.65] [--reps 5] [--warmup 2] [--views 4] [--out profiles/merge/probe_gauss.json]

Times come from device events; medians of --reps calls after --warmup."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigma", type=float, default=0.65)
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--density", type=int, default=1024)
    ap.add_argument("--sphere", type=int, default=289)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge", "probe_gauss.json"))
    a = ap.parse_args()
    import numpy as np
    from mesh2splat_amd import synth
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.score import orbit_cameras, preview_rule
    R, W, H = a.density, 1280, 720
    scene = synth.cube_sphere(a.sphere, tex_size=2048 if a.sphere >= 64 else 64)
    c = Converter(0)
    c.upload_scene(scene)
    c.set_max_gaussians(0)
    c.set_profiling(True)
    models = (("footprint", 1.0), ("gaussian", a.sigma))

    def convert():
        n = c.convert(R)
        c.to_world_units()
        return n

    def median_of(rows):
        return {k: statistics.median(r[k] for r in rows) for k in rows[0]}

    records = convert()
    res = {"scene": "c3" if a.sphere == 289 else f"cube_sphere({a.sphere})", "density": R, "records": records, "world_units": True, "level": a.level,
           "sigma": a.sigma, "reps": a.reps, "warmup": a.warmup}
    merge_rows, build_rows, counts, builds = {m: [] for m, _ in models}, {m: [] for m, _ in models}, {}, {}
    for k in range(a.warmup + a.reps):
        for m, sigma in models:
            c.set_merge_model(m, sigma)
            convert()
            counts[m] = c.merge(a.level)
            ms = c.last_merge_stage_ms()
            convert()
            builds[m] = c.lod_build()
            if k >= a.warmup:
                merge_rows[m].append(ms)
                build_rows[m].append({"build": c.last_lod_build_ms()})
    for m, _ in models:
        first = builds[m]["first"]
        res[m] = {"merge_counts": counts[m], "merge_stage_ms": median_of(merge_rows[m]), "lod_build_ms": median_of(build_rows[m])["build"],
                  "lod_nodes": builds[m]["nodes"], "lod_per_level_nodes": [first[l + 1] - first[l] for l in range(len(first) - 1)]}
    res["reduce_ratio_gaussian_to_footprint"] = res["gaussian"]["merge_stage_ms"]["reduce"] / res["footprint"]["merge_stage_ms"]["reduce"]
    res["lod_build_ratio_gaussian_to_footprint"] = res["gaussian"]["lod_build_ms"] / res["footprint"]["lod_build_ms"]

    # ---- score: half the records under each model, against the mesh render
    ctr, dist, _, _ = preview_rule(scene)
    light, inten = (ctr[0] + dist, ctr[1] + dist, ctr[2] + dist), 4.0 * dist * dist
    cams = orbit_cameras(scene, a.views, W, H, 20.0)

    def score():
        s = c.score_views(cams, c.resolution, light, inten)[1]
        return {"psnr_db": s.psnr if np.isfinite(s.psnr) else "inf", "ssim": s.ssim}

    convert()
    res["score_all_records"] = score()
    for m, sigma in models:
        c.set_merge_model(m, sigma)
        convert()
        out = c.merge_to_budget(records // 2)
        rec = c.download()
        res[m]["half"] = {"level": out["level"], "met": out["met"], "after": out["after"], "score": score(),
                          "median_largest_scale": float(np.median(np.abs(rec[:, 8:11]).max(1)))}
    c.set_merge_model("footprint")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    c.close()


if __name__ == "__main__":
    main()
