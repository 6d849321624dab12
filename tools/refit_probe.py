"""Measures the colour refit (m2s_refit_accumulate, m2s_refit_apply) on C3 at 1920 x 1080, and what it buys there.

Time: convert -> m2s_prepass_sorted -> m2s_splat + m2s_mesh_render (the two albedo planes) -> m2s_contrib_accumulate (the yardstick: the
sibling blend on the same quads in the same process) -> m2s_refit_accumulate, profiling on; then m2s_refit_apply.
Gain: the same records without refit against 1, 2 and 4 iterations of Converter.refit_views through K cameras at each training
elevation: the pooled albedo SSE (mask 3) and --score's lit PSNR, on the training cameras and on held-out ones (other elevations, another
number of views per ring, so no azimuth is shared).  Nothing is fixed in advance; the numbers go where --out says.

    python tools/refit_probe.py [--size 1920x1080] [--reps 5] [--warmup 2] [--views 8] [--out profiles/refit/probe.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TRAIN_ELEVATIONS = (-35.0, 0.0, 35.0)
HELD_OUT_ELEVATIONS = (-60.0, 17.5, 60.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    import camera
    from mesh2splat_amd import score as sc
    from mesh2splat_amd import synth
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.prepass import PrepassParams
    from mesh2splat_amd.prune import orbit_cameras
    from mesh2splat_amd.refit import RefitParams
    from mesh2splat_amd.splat import SplatParams
    R = 1024
    scene = synth.cube_sphere(289, tex_size=2048)
    conv = Converter(0)
    conv.upload_scene(scene)
    conv.convert(R)
    records = conv.num_stored
    conv.set_profiling(True)

    # ---- time -----------------------------------------------------------------------------------------------------------------------
    pp = PrepassParams(view_mat=camera.look_at((1.6, 1.1, 2.3), (0.1, 0.0, -0.1)), proj_mat=camera.perspective(45.0, W / H, 0.01, 100.0),
                       renderer_resolution=(W, H), resolution_target=R, render_mode=0)
    sp = SplatParams((W, H), 0)
    quads = conv.prepass_sorted(pp, download=False)
    conv.splat(sp, download=False)
    conv.mesh_render(pp, download=False)
    conv.contrib_begin()
    conv.refit_begin()
    contrib, refit, counts = [], [], None
    for k in range(a.warmup + a.reps):
        conv.contrib_accumulate(sp, 1.0 / 255.0)
        c = conv.last_contrib_stage_ms()
        counts = conv.refit_accumulate(RefitParams((W, H), 128))
        r = conv.last_refit_stage_ms()
        if k >= a.warmup:
            contrib.append(c)
            refit.append(r)
    med = lambda rows, key: statistics.median(r[key] for r in rows)
    res = {"scene": "c3", "density": R, "size": [W, H], "records": records, "quads": quads, "accumulate_counts": counts,
           "contrib_stage_ms": {k: med(contrib, k) for k in contrib[0]}, "refit_stage_ms": {k: med(refit, k) for k in ("setup_bin", "grouping", "blend")},
           "reps": a.reps, "warmup": a.warmup}
    res["refit_blend_over_contrib_blend"] = res["refit_stage_ms"]["blend"] / res["contrib_stage_ms"]["blend"]
    num, den = conv.download_refit()
    res["records_with_weight"] = int((den > 0).sum())
    res["max_den_bits"] = int(den.max()).bit_length()
    res["max_num_bits"] = int(abs(num).max()).bit_length()
    first = conv.refit_apply(1.0, 1.0)                         # the first call: its counters are allocated inside
    res["apply"] = dict(first, ms=conv.last_refit_stage_ms()["apply"])
    warm = []
    for k in range(a.warmup + a.reps):
        conv.refit_begin()
        conv.upload_refit(num, den)
        conv.refit_apply(1.0, 1.0)
        if k >= a.warmup:
            warm.append(conv.last_refit_stage_ms()["apply"])
    res["apply_warm_ms"] = statistics.median(warm)
    del num, den

    # ---- gain -----------------------------------------------------------------------------------------------------------------------
    conv.set_profiling(False)
    conv.convert(R)                                            # the conversion's own colours again
    train = orbit_cameras(scene, a.views, W, H, TRAIN_ELEVATIONS)
    held = orbit_cameras(scene, a.views - 3 if a.views > 4 else a.views + 1, W, H, HELD_OUT_ELEVATIONS)
    ctr, dist, _, _ = sc.preview_rule(scene)
    radius = dist * 0.41421356237309503 / 1.1                  # tan(22.5 deg): the command line's preview light
    light, intensity = (ctr[0] + 0.75 * radius, ctr[1] + 0.75 * radius, ctr[2] + 1.5 * radius), 4.0 * radius * radius

    def measure():
        out = {}
        for name, cams in (("train", train), ("held_out", held)):
            alb = conv.refit_views(cams, R, iterations=0)      # (no iteration: the pooled albedo SSE alone)
            _, pooled = conv.score_views(cams, R, light, intensity)
            out[name] = {"albedo_sse": alb["sse"][0], "albedo_pixels": alb["pixels"][0], "score_psnr_db": pooled.psnr, "score_ssim": pooled.ssim,
                         "score_sse": sum(pooled.sse), "score_pixels": pooled.pixels}
        return out

    gain = {"train_elevations": list(TRAIN_ELEVATIONS), "held_out_elevations": list(HELD_OUT_ELEVATIONS), "train_views": len(train),
            "held_out_views": len(held), "step": 1.0, "min_cover": 128, "min_weight_sum": 1.0, "after_iterations": {"0": measure()}, "per_iteration": []}
    done = 0
    for upto in (1, 2, 4):
        while done < upto:
            it = conv.refit_views(train, R, iterations=1)
            gain["per_iteration"].append({"sse_before": it["sse"][0], "sse_after": it["sse"][1], "updated": it["updated"][0],
                                          "clamped": it["clamped"][0], "no_weight": it["no_weight"][0]})
            done += 1
        gain["after_iterations"][str(upto)] = measure()
    res["gain"] = gain
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    conv.close()


if __name__ == "__main__":
    main()
