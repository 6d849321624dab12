"""Per-wave timeline of k_fused3 (the lean team kernel) on a -DM2S_TIMELINE build of the library: when workgroups start, how long the
triangle phase, the wait for the base / the other waves' entries and the strips take, how many waves are alive over time; and how far
the workgroups age in lockstep: the spread of "waves in strips" over the plateau, the triangle phase per phase class, the classes that
met on one CU (m2s_fused3.hip, phase classes; the hardware ids are recorded by builds from round 7 on); and per XCD what the dispatch
order of the runs gave it (runs, fragments) and when it ran dry (start of its last workgroup, end of its last wave).
    M2S_LIB_PATH=mesh2splat_amd/_build_tl/libm2s_hip.so python tools/timeline_fused3.py [c3|c2] [out.json]"""
import ctypes as C
import json
import os
import sys
sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import bench  # noqa: E402
from mesh2splat_amd import synth, _lib  # noqa: E402
from mesh2splat_amd.converter import Converter  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
out = sys.argv[2] if len(sys.argv) > 2 else None
n, tex, R = bench.WORKLOADS[name]
scene = synth.colocated_spheres(1, n, tex)
L = _lib.load()
c = Converter(0)
c.set_resolution_hint(R)
c.upload_scene(scene)
c.set_pipeline(os.environ.get("TL_PIPELINE", "lean"))
for _ in range(4):
    tot = c.convert(R)
L.m2s_debug_timeline_f3.restype = C.c_int
L.m2s_debug_timeline_f3.argtypes = [C.c_void_p, C.c_size_t]
L.m2s_debug_timeline_f3_clear()
c.set_profiling(True)
tot = c.convert(R)
kms = c.last_kernel_ms()
t = np.zeros((16384, 4, 8), np.uint64)
assert L.m2s_debug_timeline_f3(t.ctypes.data, t.nbytes) == 0
used = t[:, :, 0].any(axis=1)
nwg = int(np.nonzero(used)[0].max()) + 1
t = t[:nwg].astype(np.int64)
ok = t[:, 0, 0] > 0
T0 = t[ok][:, :, 0].min()
ts = (t[:, :, :6] - T0) * 10     # ns
ts[~ok] = 0
strips = t[:, :, 6] & 0xFFFFFFFF
xcc, cls_rec, hwid = (t[:, 0, 6] >> 32) & 0xF, (t[:, 0, 6] >> 40) & 0x3, (t[:, 0, 7] >> 32) & 0xFFFFFFFF
have_hw = bool(hwid[ok].any())
cls = cls_rec if have_hw else (np.arange(nwg) >> 8) & 3      # (what f3_class computes from blockIdx.x)
print(json.dumps({"workload": name, "R": R, "gaussians": int(tot), "pipeline": str(c.last_pipeline), "kernel_ms": kms, "workgroups": nwg, "with_work": int(ok.sum())}))
st, en = ts[ok][:, :, 0], ts[ok][:, :, 5]
print(f"span {en.max()} ns; workgroup starts p50 {np.percentile(st, 50):.0f} p90 {np.percentile(st, 90):.0f} max {st.max()}")
d = np.diff(ts[ok], axis=2)
lab = ["triangle phase", "wait counts/base + expand", "wait all counts", "strips", "epilogue"]
print("mean ns per phase over waves:", {lab[i]: int(d[:, :, i].mean()) for i in range(5)}, "| wave life mean", int((en - st).mean()), "p90", int(np.percentile(en - st, 90)), "max", int((en - st).max()))
print("last wave (look-back) phase 1:", {"mean": int(d[:, 3, 1].mean()), "p90": int(np.percentile(d[:, 3, 1], 90)), "max": int(d[:, 3, 1].max())})
print("strips per wave mean", float(strips[ok].mean()), "max", int(strips[ok].max()), "| ns per strip", float(d[:, :, 3].sum() / max(strips[ok].sum(), 1)))
grid = np.arange(0, en.max() + 1, 5000)
alive = [int(((st <= g) & (en > g)).sum()) for g in grid]
instrips = [int(((ts[ok][:, :, 3] <= g) & (ts[ok][:, :, 4] > g)).sum()) for g in grid]
intri = [int(((ts[ok][:, :, 0] <= g) & (ts[ok][:, :, 1] > g)).sum()) for g in grid]
inwait = [int(((ts[ok][:, :, 1] <= g) & (ts[ok][:, :, 3] > g)).sum()) for g in grid]
print("every 5 us: waves alive", alive)
print("            in the triangle phase", intri)
print("            waiting (counts, base, expansion)", inwait)
print("            in strips", instrips)
# --- lockstep figures -----------------------------------------------------------------------------------------------------------
# plateau: from the first moment (nearly) all wave slots are taken to the start of the last workgroup (after it the launch only drains)
fine = np.arange(0, en.max() + 1, 1000)
alive_f = np.array([((st <= g) & (en > g)).sum() for g in fine])
strips_f = np.array([((ts[ok][:, :, 3] <= g) & (ts[ok][:, :, 4] > g)).sum() for g in fine])
full = fine[np.argmax(alive_f >= 0.9 * alive_f.max())]
decay = st.max()
pl = strips_f[(fine >= full) & (fine <= decay)]
if len(pl):
    print(f"plateau {full / 1000:.0f} .. {decay / 1000:.0f} us (1 us samples): waves in strips min {pl.min()} max {pl.max()} mean {pl.mean():.0f} "
          f"coefficient of variation {pl.std() / pl.mean():.3f}")
# first generation: the workgroups that started before any workgroup had finished
gen1 = ok & (ts[:, :, 0].min(axis=1) < en.min())
tri_ns = (ts[:, :, 1] - ts[:, :, 0])
print("triangle phase, mean ns per class:", {int(k): int(tri_ns[ok & (cls == k)].mean()) for k in range(4) if (ok & (cls == k)).any()},
      "| first generation only:", {int(k): int(tri_ns[gen1 & (cls == k)].mean()) for k in range(4) if (gen1 & (cls == k)).any()})
print("end of the triangle phase in the first generation, mean ns after the launch's start, per class:",
      {int(k): int(ts[:, :, 1][gen1 & (cls == k)].mean()) for k in range(4) if (gen1 & (cls == k)).any()})
if have_hw:
    cu = (xcc << 8) | ((hwid >> 8) & 0xFF)          # XCC | SE, SH, CU fields of the hardware id
    per_cu = {}
    for w in np.nonzero(gen1)[0]:
        per_cu.setdefault(int(cu[w]), []).append(int(cls[w]))
    held = np.bincount([len(v) for v in per_cu.values()])
    print(f"first generation: {int(gen1.sum())} workgroups on {len(per_cu)} CUs; workgroups per CU -> CUs {dict(enumerate(held.tolist()))}; "
          f"CUs that held four distinct classes {sum(len(set(v)) == 4 for v in per_cu.values())}, three {sum(len(set(v)) == 3 for v in per_cu.values())}")
    simd = (hwid >> 4) & 3
    print("SIMD of a workgroup's first wave, first generation:", np.bincount(simd[gen1], minlength=4).tolist())
else:
    print("first generation: hardware ids not recorded by this build")
# --- per XCD: what the dispatch order gave it and when it ran dry (RunInfo, m2s_device.h; tools/xcd_balance.py is the model) --------
if have_hw:
    lb = t[:, 0, 7] & 0xFFFFFFFF                                # the unit every workgroup converted
    cnt = c.download_triangle_counts().astype(np.int64)
    per_unit = np.add.reduceat(cnt, np.arange(0, len(cnt), 256))
    n_units = len(per_unit)
    shift = next((s for s in (5, 4, 3) if n_units >= (32 << s)), 0)     # run_shift_for
    wg_end = ts[:, :, 5].max(axis=1)
    wg_start = ts[:, :, 0].min(axis=1)
    rows = []
    for x in sorted(set(xcc[ok].tolist())):
        sel = ok & (xcc == x)
        rows.append({"xcc": int(x), "dispatched_as": sorted(set((np.nonzero(sel)[0] & 7).tolist())), "workgroups": int(sel.sum()),
                     "runs": int(len(set((lb[sel] >> shift).tolist()))) if shift else 0, "fragments": int(per_unit[lb[sel]].sum()),
                     "last_workgroup_start_ns": int(wg_start[sel].max()), "last_wave_end_ns": int(wg_end[sel].max())})
    mean_f = np.mean([r["fragments"] for r in rows])
    ends = np.array([r["last_wave_end_ns"] for r in rows])
    print(f"per XCD (runs of {1 << shift} units): fragments heaviest / mean {max(r['fragments'] for r in rows) / mean_f:.4f}; "
          f"last wave ends {ends.min()} ... {ends.max()} ns (spread {ends.max() - ends.min()} ns = {100.0 * (ends.max() - ends.min()) / en.max():.1f} % of the span)")
    for r in rows:
        print(f"  XCC {r['xcc']} (workgroups h % 8 in {r['dispatched_as']}): {r['workgroups']} workgroups, {r['runs']} runs, {r['fragments']} fragments "
              f"({r['fragments'] / mean_f:.4f} of the mean); last workgroup starts {r['last_workgroup_start_ns']} ns, last wave ends {r['last_wave_end_ns']} ns")
if out:
    json.dump({"t": ts.tolist(), "strips": strips.tolist(), "lb": (t[:, :, 7] & 0xFFFFFFFF).tolist(), "class": cls.tolist(),
               "xcc": xcc.tolist(), "hw_id": hwid.tolist()}, open(out, "w"))
