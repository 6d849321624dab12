"""Measures the mesh render pass (m2s_mesh_render) against the mesh depth prepass on the same frames: upload -> m2s_mesh_render and
m2s_mesh_depth at W x H with profiling on.  The visibility stage of the render pass is the depth pass's work with an 8-byte payload;
the ratio of the two is the figure DESIGN 5.11 asks for.

    python tools/meshrender_probe.py [--scene c3|hetero|hetero_inside ...] [--size 1920x1080] [--reps 5] [--out profiles/meshrender/probe.json]

Per scene: the six counts, the pass's four stages (clear + setup + in-place, clipper + binning, tile raster, shading; median of --reps
calls after one warm-up), beside them the three stages of m2s_mesh_depth on the same frame, B_alg = 36 B per triangle + 8 B per pixel
of visibility + 32 B per pixel written and the share of 8 TB/s it corresponds to.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/meshrender_probe.py ...` for per-kernel times, and alone under `rocprofv3 --pmc ...`
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 8e12


def main():
    from meshdepth_probe import SCENES, inside_camera          # the same frames as the depth pass's probe
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", nargs="+", default=["c3", "hetero", "hetero_inside"], choices=sorted(SCENES))
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    import camera
    from mesh2splat_amd import synth
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.prepass import PrepassParams
    res = {"size": [W, H], "scenes": {}}
    med = lambda v: float(np.median(v[1:]))
    for name in a.scene:
        build, R, cam = SCENES[name]
        scene = build(synth)
        eye, ctr = cam or inside_camera(scene)
        conv = Converter(0)
        conv.upload_scene(scene)
        tris = conv.num_triangles
        pp = PrepassParams(view_mat=camera.look_at(eye, ctr), proj_mat=camera.perspective(45.0, W / H, 0.01, 100.0),
                           renderer_resolution=(W, H), near_plane=0.01, far_plane=100.0, resolution_target=R)
        conv.set_profiling(True)
        stages, walls, depth_stages = [], [], []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            counts = conv.mesh_render(pp, download=False)
            walls.append((time.perf_counter() - t0) * 1e3)
            stages.append(conv.last_mesh_render_stage_ms())
        for _ in range(a.reps + 1):
            depth_counts = conv.mesh_depth(pp, download=False)
            depth_stages.append(conv.last_mesh_depth_stage_ms())
        stage = {k: med([s[k] for s in stages]) for k in stages[0]}
        dstage = {k: med([s[k] for s in depth_stages]) for k in depth_stages[0]}
        vis_ms = stage["setup"] + stage["bin"] + stage["raster"]
        depth_ms = sum(dstage.values())
        total_ms = vis_ms + stage["shade"]
        b_alg = 36 * tris + 8 * W * H + 32 * W * H
        out = {"triangles": tris, "eye": list(eye), "centre": list(ctr), **counts, "stage_ms": stage, "visibility_ms": vis_ms,
               "mesh_render_ms": total_ms, "mesh_render_wall_ms": med(walls), "mesh_depth_stage_ms": dstage, "mesh_depth_ms": depth_ms,
               "mesh_depth_drawn": depth_counts["drawn"], "visibility_over_mesh_depth": vis_ms / depth_ms if depth_ms else None,
               "alg_bytes": b_alg, "share_of_8TBs": b_alg / HBM / (total_ms * 1e-3) if total_ms else None}
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
