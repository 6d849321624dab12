"""Measures the fidelity score's kernel (m2s_score_frames: k_score) on seeded random byte images.

    python tools/score_probe.py [--size 1920x1080 8192x8192] [--reps 20] [--out profiles/score/probe.json]

Per size, with and without the coverage planes (M2S_SCORE_NO_COVER) and with the error map: the kernel time from the context's device
events (median of --reps calls after one warm-up), the wall-clock of the whole synchronous call, B_alg = 16 bytes per pixel (8 without
coverage; + 4 with the map) and the share of 8 TB/s it corresponds to.  The images of 8192 x 8192 total 1 GiB: beyond the Infinity
Cache, so the figure is an HBM figure; at 1920 x 1080 (32 MB) repeated calls read from the cache.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/score_probe.py ...` for the kernel's own time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", nargs="+", default=["1920x1080", "8192x8192"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.score import ScoreParams
    conv = Converter(0)
    conv.set_profiling(True)
    res = {"reps": a.reps, "sizes": {}}
    med = lambda v: float(np.median(v[1:]))
    for size in a.size:
        W, H = (int(v) for v in size.split("x"))
        g = torch.Generator(device="cuda")
        g.manual_seed(W * 10000 + H)
        imgs = [torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(4)]
        torch.cuda.synchronize()
        out = {}
        for name, no_cover, want_map, per_px in (("cover", False, False, 16), ("no_cover", True, False, 8), ("cover_map", False, True, 20)):
            p = ScoreParams((W, H), 2, no_cover, want_map)
            kern, wall, r = [], [], None
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                r = conv.score_frames(p, imgs[0], imgs[1], None if no_cover else imgs[2], None if no_cover else imgs[3])
                wall.append((time.perf_counter() - t0) * 1e3)
                kern.append(conv.last_score_ms)
            b_alg = per_px * W * H
            k_ms = med(kern)
            out[name] = {"kernel_ms": k_ms, "call_wall_ms": med(wall), "alg_bytes": b_alg, "share_of_8TBs": b_alg / HBM / (k_ms * 1e-3) if k_ms else None,
                         "windows": r.windows, "pixels": r.pixels}
            print(size, name, json.dumps(out[name]))
        res["sizes"][size] = out
        del imgs
    conv.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
