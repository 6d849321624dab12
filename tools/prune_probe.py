"""Measures the contribution pass and the pruning (m2s_contrib_accumulate, m2s_prune) on C3's 2.74 M quads at 1920 x 1080: convert ->
m2s_prepass_sorted -> m2s_splat (the yardstick: its blend stage, on the same quads in the same process) -> m2s_contrib_accumulate,
profiling on; then m2s_prune — a first call, which allocates its buffers, and warm calls on the same records and accumulators put back —
against a device-to-device copy of the kept bytes.

    python tools/prune_probe.py [--size 1920x1080] [--reps 5] [--warmup 2] [--out profiles/prune/probe.json]

Stage times come from device events (m2s_last_splat_stage_ms, m2s_last_contrib_stage_ms); medians of --reps runs after --warmup."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    import torch
    import camera
    from mesh2splat_amd import synth
    from mesh2splat_amd.converter import Converter
    from mesh2splat_amd.prepass import PrepassParams
    from mesh2splat_amd.splat import SplatParams
    R = 1024
    conv = Converter(0)
    conv.upload_scene(synth.cube_sphere(289, tex_size=2048))
    conv.convert(R)
    records = conv.num_stored
    conv.set_profiling(True)
    eye = (1.6, 1.1, 2.3)
    pp = PrepassParams(view_mat=camera.look_at(eye, (0.1, 0.0, -0.1)), proj_mat=camera.perspective(45.0, W / H, 0.01, 100.0),
                       renderer_resolution=(W, H), resolution_target=R, render_mode=0)
    sp = SplatParams((W, H), 0)
    quads = conv.prepass_sorted(pp, download=False)
    conv.contrib_begin()
    blend, contrib = [], []
    for k in range(a.warmup + a.reps):
        conv.splat(sp, download=False)
        b = conv.last_splat_stage_ms()
        conv.contrib_accumulate(sp, 1.0 / 255.0)
        c = conv.last_contrib_stage_ms()
        if k >= a.warmup:
            blend.append(b)
            contrib.append(c)
    med = lambda rows, key: statistics.median(r[key] for r in rows)
    res = {"scene": "c3", "density": R, "size": [W, H], "records": records, "quads": quads, "splat_counts": conv.last_splat_counts(),
           "splat_stage_ms": {k: med(blend, k) for k in blend[0]}, "contrib_stage_ms": {k: med(contrib, k) for k in contrib[0]},
           "reps": a.reps, "warmup": a.warmup}
    res["contrib_blend_over_splat_blend"] = res["contrib_stage_ms"]["blend"] / res["splat_stage_ms"]["blend"]
    # the accumulators hold reps + warmup passes of one view: wmax is that view's, npix a multiple of it
    all_records = conv.download()
    counts = conv.prune(1.0 / 255.0, 1)
    res["prune"] = dict(counts, ms=conv.last_prune_ms)          # the first call: its flag, scan and staging buffers are allocated inside
    # warm calls: the same records back in the context's pool, one pass of the same view, the same decision
    warm = []
    for k in range(a.warmup + a.reps):
        conv.upload_records(all_records)
        conv.prepass_sorted(pp, download=False)
        conv.contrib_begin()
        conv.contrib_accumulate(sp, 1.0 / 255.0)
        again = conv.prune(1.0 / 255.0, 1)
        assert again == counts, (again, counts)
        if k >= a.warmup:
            warm.append(conv.last_prune_ms)
    res["prune_warm_ms"] = statistics.median(warm)
    del all_records
    kept_bytes = counts["kept"] * 96
    src = torch.empty(max(kept_bytes, 1), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for k in range(a.warmup + a.reps):
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            times.append(ev[0].elapsed_time(ev[1]))
    res["copy_kept_bytes_ms"] = statistics.median(times)
    res["kept_bytes"] = kept_bytes
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    conv.close()


if __name__ == "__main__":
    main()
