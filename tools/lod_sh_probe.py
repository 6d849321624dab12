"""Measures what carrying the baked SH plane (m2s_set_carry_sh) costs and what it replaces, on C3's 2.74 M records at R = 1024 in world
units with the unsigned-axis chain, 1920 x 1080:

  merge   m2s_merge at level 2, the switch on and off alternating in this one process: the three stages, m2s_last_merge_sh_ms, and the
          yardstick on the same box in the same process — a device-to-device copy that moves the bytes the reduction must move (192 n read
          + 192 n' written: a copy of half that many bytes reads and writes as much).
  build   m2s_lod_build, on and off alternating.
  cuts    m2s_lod_select for the preview camera at --factors and --tau, on a tree with the plane and on a tree without, alternating
          between two contexts; per cut the stages and their spread (min, median, max over the repetitions).
  rebake  the alternative the carried plane replaces: m2s_shadow + m2s_bake_light on the records each of those cuts selected; and
          score_baked (the viewer's own lit frame of the cut against what a 3DGS viewer shows of the plane) over --views orbit cameras
          for the carried plane and for the re-baked one.

    python tools/lod_sh_probe.py [--tau 2] [--factors 1,2,4] [--views 4] [--reps 5] [--warmup 2] [--out profiles/lod/probe_sh.json]

Stage times come from device events; medians of --reps calls after --warmup, with the extremes beside them."""
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
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--density", type=int, default=1024)
    ap.add_argument("--sphere", type=int, default=289)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lod", "probe_sh.json"))
    a = ap.parse_args()
    import torch
    from mesh2splat_amd import lod, synth
    from mesh2splat_amd.bake import BakeParams
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.score import camera_from_eye, orbit_cameras, orbit_eye, preview_rule
    R, W, H = a.density, 1920, 1080
    scene = synth.cube_sphere(a.sphere, tex_size=2048 if a.sphere >= 64 else 64)
    on = Converter(0)                    # converts, bakes; its trees carry the plane
    off = Converter(0)                   # adopts the same records; its trees do not
    on.upload_scene(scene)
    on.set_max_gaussians(0)
    on.set_profiling(True)
    off.set_profiling(True)
    ctr, dist, near, far = preview_rule(scene)
    light = (ctr[0] + dist, ctr[1] + dist, ctr[2] + dist)
    inten = 4.0 * dist * dist
    plain_bake = BakeParams(use_shadows=False)

    def camera(f):
        return camera_from_eye(orbit_eye(ctr, dist * f, 0, 1), ctr, near, far * f, W, H)

    def fresh(plane=True):
        """the conversion in world units on `on`, with a plane of the records (its contents do not change what a merge costs)"""
        n = on.convert(R)
        on.to_world_units()
        if plane:
            _, lp = camera(1.0).frame_params(on.resolution, light, inten)
            on.bake_light(plain_bake, lp, download=False)
        return n

    n = fresh()
    res = {"scene": "c3" if a.sphere == 289 else f"cube_sphere({a.sphere})", "density": R, "size": [W, H], "records": n, "reps": a.reps, "warmup": a.warmup,
           "world_units": True, "unsigned_axis": True, "tau_px": a.tau}

    # ---- merge at level 2, on / off alternating
    rows = {True: [], False: []}
    counts = None
    for k in range(a.warmup + a.reps):
        for sw in ((True, False) if k % 2 == 0 else (False, True)):
            fresh()
            on.carry_sh = sw
            got = on.merge(2, 4, 0.5, unsigned_axis=True)
            assert counts is None or got == counts
            counts = got
            ms = on.last_merge_stage_ms()
            ms["sh"] = on.last_merge_sh_ms
            assert (ms["sh"] > 0) == sw and bool(on.device_sh) == sw
            if k >= a.warmup:
                rows[sw].append(ms)
    moved = 192 * (counts["before"] + counts["after"])
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    copies = []
    for k in range(a.warmup + a.reps):
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            copies.append(ev[0].elapsed_time(ev[1]))
    del src, dst
    sh_ms = statistics.median(r["sh"] for r in rows[True])
    res["merge_level_2"] = {"counts": counts, "bytes_the_reduction_moves": moved,
                            "on": {key: spread([r[key] for r in rows[True]]) for key in rows[True][0]},
                            "off": {key: spread([r[key] for r in rows[False]]) for key in rows[False][0]},
                            "d2d_copy_of_half_those_bytes_ms": spread(copies), "sh_over_copy": sh_ms / statistics.median(copies)}
    print(json.dumps({"merge_level_2": res["merge_level_2"]}), flush=True)

    # ---- m2s_lod_build, on / off alternating
    rows = {True: [], False: []}
    build = None
    for k in range(a.warmup + a.reps):
        for sw in ((True, False) if k % 2 == 0 else (False, True)):
            fresh()
            on.carry_sh = sw
            got = on.lod_build(unsigned_axis=True)
            assert build is None or got == build
            build = got
            assert bool(on.device_lod_sh) == sw
            if k >= a.warmup:
                rows[sw].append(on.last_lod_build_ms)
    first = build["first"]
    res["build"] = {"counts": {k: v for k, v in build.items() if k != "first"}, "per_level_nodes": [first[l + 1] - first[l] for l in range(len(first) - 1)],
                    "plane_bytes": 192 * build["nodes"], "on_ms": spread(rows[True]), "off_ms": spread(rows[False])}
    print(json.dumps({"build": res["build"]}), flush=True)

    # ---- the two trees side by side: `off` adopts the records and builds without a plane, `on` bakes with shadows and builds with it
    fresh(plane=False)
    off.set_records(on.device_records, n, on.resolution)
    assert off.lod_build(unsigned_axis=True) == build and not off.device_lod_sh
    pp1, lp1 = camera(1.0).frame_params(on.resolution, light, inten)
    on.carry_sh = True
    on.shadow(pp1, lp1, download=False)
    full_shadow_ms = on.last_shadow_ms
    on.bake_light(BakeParams(), lp1, download=False)
    res["bake_of_every_record_ms"] = {"shadow": full_shadow_ms, "bake": on.last_bake_ms}
    assert on.lod_build(unsigned_axis=True) == build and on.device_lod_sh
    views = orbit_cameras(scene, a.views, W, H)
    res["cuts"] = []
    for f in [float(v) for v in a.factors.split(",")]:
        cam = camera(f)
        eye, focal = lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, H)
        rows = {"on": [], "off": []}
        counts = None
        for k in range(a.warmup + a.reps):
            for name, c in ((("on", on), ("off", off)) if k % 2 == 0 else (("off", off), ("on", on))):
                got = c.lod_select(eye, focal, a.tau, cam.near)
                assert counts is None or got == counts
                counts = got
                ms = c.last_lod_select_stage_ms()
                ms["total"] = ms["sweep"] + ms["scan_ids"] + ms["compact"]
                if k >= a.warmup:
                    rows[name].append(ms)
        row = {"factor": f, "counts": counts, "on": {key: spread([r[key] for r in rows["on"]]) for key in rows["on"][0]},
               "off": {key: spread([r[key] for r in rows["off"]]) for key in rows["off"][0]}}
        # the carried plane of this cut against the viewer's lit frame, then the alternative: shadow + bake of the selected records
        assert on.sh_plane_info()["rows"] == counts["selected"]

        def scores():
            out = []
            for v in views:
                pp, lp = v.frame_params(on.resolution, light, inten)
                s = on.score_baked(pp, lp)
                out.append({"psnr_db": s.psnr, "ssim": s.ssim})
            return out

        row["score_baked_carried"] = scores()
        pp, lp = cam.frame_params(on.resolution, light, inten)
        rebake = []
        for k in range(a.warmup + a.reps):
            on.shadow(pp, lp, download=False)
            t = {"shadow": on.last_shadow_ms}
            on.bake_light(BakeParams(), lp, download=False)
            t["bake"] = on.last_bake_ms
            t["total"] = t["shadow"] + t["bake"]
            if k >= a.warmup:
                rebake.append(t)
        row["rebake_selected_ms"] = {key: spread([r[key] for r in rebake]) for key in rebake[0]}
        row["score_baked_rebaked"] = scores()
        row["psnr_db_carried_minus_rebaked"] = [x["psnr_db"] - y["psnr_db"] for x, y in zip(row["score_baked_carried"], row["score_baked_rebaked"])]
        res["cuts"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    on.close()
    off.close()


if __name__ == "__main__":
    main()
