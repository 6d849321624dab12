"""Measures the compact .ply export (m2s_export_ply_compact) on C3's 2.74 M records (cube_sphere(289) at R = 1024): the four stages —
box + keys, sort, pack (device events), download + write (host clock) — and the file size, medians of --reps runs after --warmup; and,
for comparison, the wall time of export_ply in formats 0 and 1 from the same process to the same directory.

    python tools/compact_probe.py [--reps 5] [--warmup 2] [--dir /tmp] [--plane] [--out profiles/compact/probe.json]

--plane: a depth sort first leaves the 16-byte position plane behind, so that the key kernel reads it instead of the records."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default="")
    ap.add_argument("--plane", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import camera
    from mesh2splat_amd import synth
    from mesh2splat_amd.converter import Converter
    R = 1024
    conv = Converter(0)
    conv.upload_scene(synth.cube_sphere(289, tex_size=2048))
    conv.convert(R)
    res = {"scene": "c3", "density": R, "records": conv.num_stored, "reps": a.reps, "warmup": a.warmup}
    if a.plane:
        conv.sort_by_depth(camera.look_at((1.6, 1.1, 2.3), (0.1, 0.0, -0.1)), download=False)
    res["position_plane"] = conv.positions_ready
    with tempfile.TemporaryDirectory(dir=a.dir or None) as d:
        path = os.path.join(d, "probe.ply")
        stages, wall = [], []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            info = conv.export_ply_compact(path, 0.65)
            t1 = time.perf_counter()
            if k >= a.warmup:
                stages.append(info["stage_ms"])
                wall.append((t1 - t0) * 1e3)
        res.update(rows=info["rows"], chunks=info["chunks"], skipped=info["skipped"], bytes=info["bytes"],
                   bytes_per_row=info["bytes"] / max(info["rows"], 1), stage_ms={s: statistics.median(r[s] for r in stages) for s in stages[0]},
                   wall_ms=statistics.median(wall))
        for fmt in (0, 1):
            wall = []
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                conv.export_ply(path, fmt, 0.65)
                t1 = time.perf_counter()
                if k >= a.warmup:
                    wall.append((t1 - t0) * 1e3)
            res[f"format{fmt}"] = {"wall_ms": statistics.median(wall), "bytes": os.path.getsize(path)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    conv.close()


if __name__ == "__main__":
    main()
