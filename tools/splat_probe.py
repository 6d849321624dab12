"""Measures the splat pass (m2s_splat) on real frames: convert -> m2s_prepass -> m2s_sort_prepass -> m2s_splat at W x H, profiling on.

    python tools/splat_probe.py [--scene c3|hetero|c5 ...] [--size 1920x1080] [--reps 5] [--mode 0] [--out profiles/splat/probe.json]

Per scene: quads drawn, (tile, quad) pairs, fragments blended, the three stages (setup + bin, grouping, blend; median of --reps calls
after one warm-up), the blend's fragment rate, and the tile load (longest list, mean non-empty list).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/splat_probe.py ...` for per-kernel times, and alone under `rocprofv3 --pmc ...`
(one counter set per run) for the counters."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", nargs="+", default=["c3", "hetero"], choices=sorted(SCENES))
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    import camera
    from mesh2splat_amd import synth
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.prepass import PrepassParams
    from mesh2splat_amd.splat import SplatParams
    res = {"size": [W, H], "mode": a.mode, "camera": "perspective 45 deg, eye (1.6,1.1,2.3) -> (0.1,0,-0.1)", "scenes": {}}
    for name in a.scene:
        build, R = SCENES[name]
        scene = build(synth)
        conv = Converter(0)
        if name == "c5":
            conv.set_max_gaussians(0)
        conv.upload_scene(scene)
        total = conv.convert(R)
        pp = PrepassParams(view_mat=camera.look_at((1.6, 1.1, 2.3), (0.1, 0.0, -0.1)), proj_mat=camera.perspective(45.0, W / H, 0.01, 100.0),
                           renderer_resolution=(W, H), resolution_target=R)
        vis = conv.prepass(pp, download=False)
        n = conv.sort_prepass(download=False)
        conv.set_profiling(True)
        stages, walls = [], []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            conv.splat(SplatParams((W, H), a.mode), download=False)
            walls.append((time.perf_counter() - t0) * 1e3)
            stages.append(conv.last_splat_stage_ms())
        counts = conv.last_splat_counts()
        med = {k: float(np.median([s[k] for s in stages[1:]])) for k in stages[0]}
        # tile loads from the restatement's setup (the kernel's own pairs: checked equal in tests/test_gpu_splat.py)
        import splat_ref
        tc = splat_ref.tile_counts(splat_ref.setup(conv.sort_prepass(), W, H)) if n < 4_000_000 else None
        r = {"records": int(total), "quads": int(n), "visible": int(vis), **counts, "stage_ms": med,
             "splat_ms": float(sum(med.values())), "call_ms_wall": float(np.median(walls[1:])),
             "fragments_per_s_blend": counts["fragments"] / (med["blend"] * 1e-3) if med["blend"] > 0 else None}
        if tc is not None:
            nz = tc[tc > 0]
            r["tiles"] = {"n": int(tc.size), "non_empty": int(nz.size), "longest": int(tc.max()), "mean_non_empty": float(nz.mean()) if nz.size else 0.0}
        res["scenes"][name] = r
        print(name, json.dumps(r))
        conv.close()
        del scene
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
