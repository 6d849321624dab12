"""Measures the mesh depth prepass (m2s_mesh_depth) and what it buys the frame: upload -> convert -> m2s_mesh_depth at W x H with
profiling on, then the frame (m2s_prepass_sorted + m2s_splat) with and without the occlusion test.

    python tools/meshdepth_probe.py [--scene c3|hetero|hetero_inside ...] [--size 1920x1080] [--reps 5] [--out profiles/meshdepth/probe.json]

Per scene: the five counts, the pass's three stages (clear + setup + in-place, clipper + binning, tile raster; median of --reps calls
after one warm-up), B_alg = 36 B per triangle + 4 W H and the share of 8 TB/s it corresponds to, and the wall-clock of the frame with
and without the mesh as occluder (median of --reps after a warm-up) with the quads each splats.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/meshdepth_probe.py ...` for per-kernel times, and alone under `rocprofv3 --pmc ...`
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

VIEWER = ((1.6, 1.1, 2.3), (0.1, 0.0, -0.1))          # bench.py's viewer camera
SCENES = {  # name: (builder, R, (eye, centre))
    "c3": (lambda s: s.cube_sphere(289, tex_size=2048), 1024, VIEWER),
    "hetero": (lambda s: s.sponza_like(), 1024, VIEWER),
    "hetero_inside": (lambda s: s.sponza_like(), 1024, None),     # a camera inside the scene: the floor crosses the near plane
}
HBM = 8e12


def inside_camera(scene):
    lo = np.min([m.vertices[:, 0:3].min(0) for m in scene.meshes], 0)
    hi = np.max([m.vertices[:, 0:3].max(0) for m in scene.meshes], 0)
    c = (lo + hi) / 2
    eye = (float(c[0]), float(lo[1] + 0.25 * (hi[1] - lo[1])), float(c[2]))
    return eye, (float(hi[0]), eye[1] * 0.9, float(c[2] + 0.1 * (hi[2] - lo[2])))


def main():
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
    from mesh2splat_amd.splat import SplatParams
    res = {"size": [W, H], "scenes": {}}
    med = lambda v: float(np.median(v[1:]))
    for name in a.scene:
        build, R, cam = SCENES[name]
        scene = build(synth)
        eye, ctr = cam or inside_camera(scene)
        conv = Converter(0)
        conv.upload_scene(scene)
        conv.convert(R)
        tris = conv.num_triangles
        pp = PrepassParams(view_mat=camera.look_at(eye, ctr), proj_mat=camera.perspective(45.0, W / H, 0.01, 100.0),
                           renderer_resolution=(W, H), resolution_target=R)
        conv.set_profiling(True)
        stages, walls = [], []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            counts = conv.mesh_depth(pp, download=False)
            walls.append((time.perf_counter() - t0) * 1e3)
            stages.append(conv.last_mesh_depth_stage_ms())
        stage = {k: med([s[k] for s in stages]) for k in stages[0]}
        total_ms = sum(stage.values())
        b_alg = 36 * tris + 4 * W * H
        frame = {}
        for key, p in (("without", pp), ("with", conv._with_device_mesh_depth(pp))):
            t, quads = [], 0
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                if key == "with":
                    conv.mesh_depth(pp, download=False)
                quads = conv.prepass_sorted(p, download=False)
                conv.splat(SplatParams((W, H), 0), download=False)
                t.append((time.perf_counter() - t0) * 1e3)
            frame[key] = {"wall_ms": med(t), "quads": int(quads)}
        out = {"triangles": tris, "records": conv.num_stored, "eye": list(eye), "centre": list(ctr), **counts, "stage_ms": stage,
               "mesh_depth_ms": total_ms, "mesh_depth_wall_ms": med(walls), "alg_bytes": b_alg,
               "share_of_8TBs": b_alg / HBM / (total_ms * 1e-3) if total_ms else None,
               "frame_prepass_sorted_plus_splat": frame}
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
