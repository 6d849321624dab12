#!/usr/bin/env python
"""BASELINE config 3 through k_fused3 and nothing else: the process to put under `rocprofv3 --pmc ...` (one counter set per run, no
tracing beside it) or `rocprofv3 --kernel-trace --stats` when only this kernel is of interest (the per-plane traffic table).

    python tools/fused3_c3_probe.py [--launches 20] [--check]

The library is the one M2S_LIB_PATH names (A/B and measurement builds), else the package's.  Prints one JSON line: the counter, the
pipeline that ran, whether the strips gathered from the upload's vertex table (the indexed instance), whether the triangle phase read the upload's
geometry planes (the kGeo instance) and — with --check — a CRC of the
records (compare it with the shipping build's to see that a measurement build writes the same bytes).
"""
import argparse
import json
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mesh2splat_amd import synth                      # noqa: E402
from mesh2splat_amd.converter import Converter        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    scene = synth.colocated_spheres(1, 289, 2048)      # 1 002 252 triangles, three 2048^2 maps
    with Converter(0) as c:
        c.set_pipeline("lean")
        c.set_max_gaussians(0)
        c.upload_scene(scene)
        total = 0
        for _ in range(a.launches):
            total = c.convert(1024)
        out = {"total": total, "pipeline": c.last_pipeline, "launches": a.launches, "vertex_table": c.vertex_table(), "geo_planes": c.geo_planes()}
        if a.check:
            out["crc32"] = "%08x" % zlib.crc32(c.download().tobytes())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
