"""Measures what m2s_lod_blend costs and what it buys, on C3's 2.74 M records at R = 1024 in world units with the unsigned-axis tree
(a baked plane carried, so that all three kernels run) and the preview camera, 1920 x 1080:

  time    m2s_lod_select at --tau for the preview camera at --factors (the three cuts of profiles/lod/probe_sh.json), then
          m2s_lod_blend with band 1 on each: its three kernels, beside the cut's own stages and a device-to-device copy of the bytes the
          blend writes (96 + 192 per record).
  pops    for --keys switch keys of the preview camera — the tau_px m2s_lod_select_budget returns for budgets spread between the last
          level and the leaves: the smallest key at which the count drops — the frame one key below against the frame at the key
          (score_frames over every pixel), for the plain cut and for the cut blended with bands 1 and 0.25.  The plain figure is the
          pop; what is left with band 1 is the residual of the alpha limit (m coincident copies of a parent against the parent drawn
          once) plus rounding.

    python tools/lod_blend_probe.py [--tau 2] [--factors 1,2,4] [--keys 10] [--reps 5] [--warmup 2] [--out profiles/lod/probe_blend.json]

Times come from device events; medians of --reps calls after --warmup, with the extremes beside them."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tau", type=float, default=2.0)
    ap.add_argument("--factors", default="1,2,4")
    ap.add_argument("--keys", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--density", type=int, default=1024)
    ap.add_argument("--sphere", type=int, default=289)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lod", "probe_blend.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from mesh2splat_amd import lod, synth
    from mesh2splat_amd.bake import BakeParams
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.score import ScoreParams, camera_from_eye, orbit_eye, preview_rule
    R, W, H = a.density, 1920, 1080
    scene = synth.cube_sphere(a.sphere, tex_size=2048 if a.sphere >= 64 else 64)
    c = Converter(0)
    c.upload_scene(scene)
    c.set_max_gaussians(0)
    c.set_profiling(True)
    ctr, dist, near, far = preview_rule(scene)
    light = (ctr[0] + dist, ctr[1] + dist, ctr[2] + dist)
    inten = 4.0 * dist * dist

    def camera(f):
        return camera_from_eye(orbit_eye(ctr, dist * f, 0, 1), ctr, near, far * f, W, H)

    n = c.convert(R)
    c.to_world_units()
    _, lp = camera(1.0).frame_params(c.resolution, light, inten)
    c.carry_sh = True
    c.bake_light(BakeParams(use_shadows=False), lp, download=False)
    build = c.lod_build(unsigned_axis=True)
    first = build["first"]
    res = {"scene": "c3" if a.sphere == 289 else f"cube_sphere({a.sphere})", "density": R, "size": [W, H], "records": n, "reps": a.reps,
           "warmup": a.warmup, "world_units": True, "unsigned_axis": True, "tau_px": a.tau, "nodes": build["nodes"],
           "per_level_nodes": [first[l + 1] - first[l] for l in range(len(first) - 1)]}

    # ---- time: the cut, the blend and its kernels, a copy of the bytes the blend writes
    res["cuts"] = []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for f in [float(v) for v in a.factors.split(",")]:
        cam = camera(f)
        eye, focal = lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H)
        cut_rows, blend_rows, counts, bcounts = [], [], None, None
        for k in range(a.warmup + a.reps):
            counts = c.lod_select(eye, focal, a.tau, cam.near)
            cut = c.last_lod_select_stage_ms()
            cut["total"] = cut["sweep"] + cut["scan_ids"] + cut["compact"]
            bcounts = c.lod_blend(eye, focal, a.tau, cam.near, 1.0)
            ms = c.last_lod_blend_stage_ms()
            ms["total"] = c.last_lod_blend_ms()
            if k >= a.warmup:
                cut_rows.append(cut)
                blend_rows.append(ms)
        written = (96 + 192) * counts["selected"]
        src = torch.empty(written, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        copies = []
        for k in range(a.warmup + a.reps):
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            torch.cuda.synchronize()
            if k >= a.warmup:
                copies.append(ev[0].elapsed_time(ev[1]))
        del src, dst
        t = c.download_lod_blend_t()
        row = {"factor": f, "selected": counts["selected"], "per_level": counts["per_level"], "blend_counts": bcounts,
               "t_mean": float(t.mean()) if t.size else 0.0, "bytes_written": written,
               "bytes_read_bound": (44 + 104 + 192) * counts["selected"] + (128 + 192) * bcounts["blended"],
               "cut_ms": {key: spread([r[key] for r in cut_rows]) for key in cut_rows[0]},
               "blend_ms": {key: spread([r[key] for r in blend_rows]) for key in blend_rows[0]},
               "d2d_copy_of_the_bytes_written_ms": spread(copies)}
        res["cuts"].append(row)
        print(json.dumps(row), flush=True)

    # ---- pops: the frame one key below a switch against the frame at it, plain and blended
    cam = camera(1.0)
    eye, focal = lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H)
    pp, lp = cam.frame_params(c.resolution, light, inten)
    sp = ScoreParams(resolution=(W, H), mask_mode=0, no_cover=True)
    last, leaves = first[-1] - first[-2], first[1]

    def frame(tau, band):
        got = c.lod_select(eye, focal, tau, cam.near, blend=band)
        img = torch.from_numpy(np.ascontiguousarray(c.render_frame(pp, lp))).cuda()
        return got, img

    def score(x, y):
        s = c.score_frames(sp, a=x, b=y)
        return {"psnr_db": s.psnr if np.isfinite(s.psnr) else "inf", "max_abs": list(s.max_abs), "sad": list(s.sad)}

    res["pops"] = []
    for k in range(a.keys):
        budget = int(last + (leaves - last) * (k + 1) / (a.keys + 1))
        hit = c.lod_select_budget(eye, focal, budget, near=cam.near, dry_run=True)
        tau = float(np.float32(hit["tau_px"]))
        below = float(np.nextafter(np.float32(tau), np.float32(0)))
        row = {"budget": budget, "tau_px": tau, "tau_px_below": below, "selected": hit["selected"], "selected_below": hit["selected_finer"]}
        for name, band in (("plain", None), ("band_1", 1.0), ("band_0.25", 0.25)):
            lo, img_lo = frame(below, band)
            hi, img_hi = frame(tau, band)
            row[name] = score(img_lo, img_hi)
            if band is not None:
                row[name]["blended_below"] = lo["blend"]["blended"]
        # the alpha limit: below the switch the children that reached their parent (band 1, t ~ 1) are m coincident copies of it;
        # at the switch the parent is drawn once.  band 1's figure above IS that residual plus rounding: the plain figure is the pop.
        res["pops"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    c.close()


if __name__ == "__main__":
    main()
