"""Measures the shadow and relighting passes (m2s_shadow, m2s_relight) on real frames: convert -> m2s_prepass -> m2s_sort_prepass ->
m2s_splat -> m2s_shadow -> m2s_relight at W x H, profiling on.

    python tools/light_probe.py [--scene c3|hetero|c5 ...] [--size 1920x1080] [--shadow 1024] [--reps 5] [--out profiles/light/probe.json]

Per scene: quads per cube face, (tile, quad) pairs, texel updates sent, the shadow pass's three stages (stage A, setup + bin, raster)
and the relighting pass (median of --reps calls after one warm-up), their algorithmic bytes — shadow: 96 B read per record + 48 B
written and read per surviving quad + 4 B per cube texel; relight: 24 B read + 4 B written per pixel — and the share of 8 TB/s those
correspond to.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/light_probe.py ...` for per-kernel times, and alone
under `rocprofv3 --pmc ...` (one counter set per run) for the counters."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENES = {  # name: (builder, R) — the BASELINE workloads the rest of the project measures
    "c3": (lambda s: s.cube_sphere(289, tex_size=2048), 1024),
    "hetero": (lambda s: s.sponza_like(), 1024),
    "c5": (lambda s: s.c5_scene(1021, 4096), 2048),
}
HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", nargs="+", default=["c3", "hetero"], choices=sorted(SCENES))
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--shadow", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--light", default="1.0,2.5,1.5,20")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    lx, ly, lz, inten = (float(v) for v in a.light.split(","))
    import camera
    from mesh2splat_amd import synth
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.light import LightParams
    from mesh2splat_amd.prepass import PrepassParams
    from mesh2splat_amd.splat import SplatParams
    eye = (1.6, 1.1, 2.3)
    res = {"size": [W, H], "shadow_resolution": a.shadow, "light": [lx, ly, lz, inten],
           "camera": "perspective 45 deg, eye (1.6,1.1,2.3) -> (0.1,0,-0.1)", "scenes": {}}
    for name in a.scene:
        build, R = SCENES[name]
        conv = Converter(0)
        if name == "c5":
            conv.set_max_gaussians(0)
        conv.upload_scene(build(synth))
        conv.convert(R)
        records = conv.num_stored
        pp = PrepassParams(view_mat=camera.look_at(eye, (0.1, 0.0, -0.1)), proj_mat=camera.perspective(45.0, W / H, 0.01, 100.0),
                           renderer_resolution=(W, H), resolution_target=R, render_mode=6)
        lp = LightParams((lx, ly, lz), (1.0, 1.0, 1.0), inten, eye, 0.01, 100.0, 6, (W, H), a.shadow, False)
        conv.prepass(pp, download=False)
        conv.sort_prepass(download=False)
        conv.splat(SplatParams((W, H), 6), download=False)
        conv.set_profiling(True)
        sh, rl, walls = [], [], []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            conv.shadow(pp, lp, download=False)
            t1 = time.perf_counter()
            conv.relight(lp, download=False)
            walls.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
            sh.append(conv.last_shadow_stage_ms())
            rl.append(conv.last_relight_ms)
        med = lambda v: float(np.median(v[1:]))
        counts = conv.last_shadow_counts()
        quads = sum(counts["quads_per_face"])
        stage = {k: med([s[k] for s in sh]) for k in sh[0]}
        shadow_ms, relight_ms = sum(stage.values()), med(rl)
        b_shadow = 96 * records + 96 * quads + 4 * 6 * a.shadow * a.shadow
        b_relight = 28 * W * H
        out = {"records": records, **counts, "shadow_stage_ms": stage, "shadow_ms": shadow_ms, "relight_ms": relight_ms,
               "shadow_wall_ms": med([w[0] for w in walls]), "relight_wall_ms": med([w[1] for w in walls]),
               "shadow_alg_bytes": b_shadow, "relight_alg_bytes": b_relight,
               "shadow_share_of_8TBs": b_shadow / HBM / (shadow_ms * 1e-3) if shadow_ms else None,
               "relight_share_of_8TBs": b_relight / HBM / (relight_ms * 1e-3) if relight_ms else None}
        res["scenes"][name] = out
        print(name, json.dumps(out))
        conv.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
