"""-m gpu: m2s_prune / Converter.prune / .prune_views — the kept set against the downloaded accumulators, the compaction (records, the baked
plane, adopted records), the lossless invariant of the albedo plane, the occlusion of one wall by another against the CPU restatement,
and nested spheres through orbit cameras."""
import numpy as np
import pytest

import contrib_ref as cr
import prune_cases as pc
from mesh2splat_amd import synth
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prune import orbit_cameras
from mesh2splat_amd.scene import Mesh, Scene
from mesh2splat_amd.splat import SplatParams

pytestmark = pytest.mark.gpu
R, W, H = 64, 128, 128
CW = 1.0 / 255.0


def nested_spheres():
    outer = synth.cube_sphere_vertices(10, 1.0)
    inner = synth.cube_sphere_vertices(8, 0.5)
    return Scene([Mesh(name="outer", vertices=outer, base_color=(0.8, 0.6, 0.4, 1.0)), Mesh(name="inner", vertices=inner, base_color=(0.2, 0.4, 0.9, 1.0))])


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def accumulate(conv, cams):
    conv.contrib_begin()
    for cam in cams:
        pp, _ = cam.frame_params(R, (0, 0, 0), 0.0)
        assert conv.prepass_sorted(pp, download=False) > 0 and conv.device_sorted_sources
        conv.contrib_accumulate(SplatParams((W, H), 0), CW)
    return conv.download_contrib()


def test_kept_set_order_counts_sh_plane(conv):
    scene = nested_spheres()
    conv.upload_scene(scene)
    n = conv.convert(R)
    rec = conv.download()
    sh = conv.bake_light(BakeParams(use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)))
    cams = orbit_cameras(scene, 2, W, H, (0.0, 40.0))
    w, k = accumulate(conv, cams)
    tau, m = 0.05, 3
    keep = (w > np.float32(tau)) & (k >= m)
    assert 0 < keep.sum() < n
    counts = conv.prune(tau, m)
    assert counts == {"before": n, "kept": int(keep.sum()), "dropped_weight": int((~(w > np.float32(tau))).sum()),
                      "dropped_pixels": int(((w > np.float32(tau)) & (k < m)).sum())}
    assert counts["kept"] + counts["dropped_weight"] + counts["dropped_pixels"] == n and conv.num_stored == counts["kept"]
    assert np.array_equal(conv.download().view(np.uint32), rec[keep].view(np.uint32))          # canonical order, byte-identical
    assert np.array_equal(conv.download_sh().view(np.uint32), sh[keep].view(np.uint32))
    # what was derived from the old records is gone; the resolutionTarget is kept (the export still works out its scale)
    assert not conv.device_sorted_sources and not conv.device_contrib(0)
    with pytest.raises(Exception):
        conv.prune(tau, m)
    w2, k2 = accumulate(conv, cams)
    assert w2.size == counts["kept"]


def test_adopted_records_are_compacted_into_the_pool(conv):
    import torch
    scene = nested_spheres()
    conv.upload_scene(scene)
    n = conv.convert(R)
    rec = conv.download()
    mine = torch.from_numpy(rec.copy()).cuda()
    conv.set_records(mine.data_ptr(), n, R)
    w, k = accumulate(conv, orbit_cameras(scene, 2, W, H, (10.0,)))
    keep = (w > np.float32(0.02)) & (k >= 1)
    counts = conv.prune(0.02, 1)
    assert counts["kept"] == int(keep.sum()) and conv.device_records != mine.data_ptr()
    assert np.array_equal(mine.cpu().numpy().view(np.uint32), rec.view(np.uint32))            # the caller's memory is not written
    assert np.array_equal(conv.download().view(np.uint32), rec[keep].view(np.uint32))


def test_lossless_at_zero_thresholds(conv):
    """min_weight = 0, min_pixels = 0 drops exactly the records whose every fragment has w = 0: they add nothing to the albedo plane, and
    the compaction and the sort are stable — attachment 2 of every view is byte-identical before and after.  (The exception the pin in
    include/m2s.h names — a record of opacity exactly 0 or NaN, whose fragments have w = 0 and still add colour — cannot occur here:
    every record of this scene has opacity 1.)"""
    scene = nested_spheres()
    conv.upload_scene(scene)
    n = conv.convert(R)
    cams = orbit_cameras(scene, 3, W, H, (15.0,))

    def albedo():
        out = []
        for cam in cams:
            pp, _ = cam.frame_params(R, (0, 0, 0), 0.0)
            conv.prepass_sorted(pp, download=False)
            planes, _ = conv.splat(SplatParams((W, H), 0))
            out.append(planes[2])
        return out

    before = albedo()
    w, k = accumulate(conv, cams)
    counts = conv.prune(0.0, 0)
    assert counts["kept"] == int((w > 0).sum()) and 0 < counts["kept"] < n and counts["dropped_pixels"] == 0
    after = albedo()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert before[0][..., 3].max() == 255
    print(f"lossless: {n} -> {counts['kept']} records ({100.0 * (n - counts['kept']) / n:.1f} % dropped)")


def test_occlusion_drops_exactly_the_back_wall(conv, oracle):
    """Two parallel walls, the smaller one behind the larger (prune_cases.two_walls), R = 32, 96 x 96, gaussian_std = 1.0, seen from in
    front through a view pitched by 5 degrees (the exactly head-on view is degenerate for flat isotropic Gaussians:
    tests/test_contrib_cpu.py).  FIRST the restatement alone — contrib_ref on the oracle's prepass of these records in depth order —
    must separate the walls at tau = 0.05 with the bar to spare on either side: every back-wall record below tau - W_BAR (it gives
    them all exactly 0: the front wall saturates every pixel they reach), every front-wall record above tau + W_BAR (its minimum is
    0.15).  THEN the device chain m2s_prepass_sorted (sources) -> k_splat_contrib -> m2s_prune: per record within the bars of the
    restatement, and the pruned set is the front wall, byte for byte."""
    tau = 0.05
    W, H = pc.WALL_SIZE
    conv.upload_scene(pc.two_walls())
    n = conv.convert(pc.WALL_R)
    rec = conv.download()
    front = rec[:, 2] > 0
    assert front.sum() == 32 * 32 and (~front).sum() == 26 * 26 and np.array_equal(np.unique(rec[:, 2]), [-0.5, 0.5])
    p = pc.wall_params()
    quads, src = pc.sorted_with_sources(oracle, p, rec)
    ref = cr.per_record(cr.contrib(quads, W, H, CW, cr.W_BAR), src, n)
    rw = ref["wmax"].view(np.float32)
    print(f"restatement: back wall max wmax = {rw[~front].max():.4g}, front wall min wmax = {rw[front].min():.4g}")
    assert rw[~front].max() < tau - cr.W_BAR and rw[front].min() > tau + cr.W_BAR
    # the device
    conv.contrib_begin()
    assert conv.prepass_sorted(p, download=False) == n
    conv.contrib_accumulate(SplatParams((W, H), 0), CW)
    w, k = conv.download_contrib()
    dw = np.abs(w.astype(np.float64) - rw.astype(np.float64))
    print(f"device: max |d wmax| = {dw.max():.3g}; back wall max wmax = {w[~front].max():.4g}, front wall min wmax = {w[front].min():.4g}")
    assert dw.max() <= cr.W_BAR and ((ref["n_lo"] <= k) & (k <= ref["n_hi"])).all()
    counts = conv.prune(tau, 0)
    assert counts == {"before": n, "kept": int(front.sum()), "dropped_weight": int((~front).sum()), "dropped_pixels": 0}
    assert np.array_equal(conv.download().view(np.uint32), rec[front].view(np.uint32))


def test_nested_spheres_prune_views_and_score(conv):
    scene = nested_spheres()
    conv.upload_scene(scene)
    n = conv.convert(R)
    light = (2.0, 2.5, 3.0)
    score_cams = orbit_cameras(scene, 3, W, H, (20.0,))
    _, before = conv.score_views(score_cams, R, light, 30.0, shadow_resolution=128)
    counts = conv.prune_views(orbit_cameras(scene, 6, 2 * W, 2 * H, (-30.0, 30.0)), R, (W, H))
    _, after = conv.score_views(score_cams, R, light, 30.0, shadow_resolution=128)
    assert counts["before"] == n and counts["kept"] + counts["dropped_weight"] + counts["dropped_pixels"] == n
    assert conv.num_stored == counts["kept"] and 0 < counts["kept"] < n
    print(f"nested spheres: {counts}; psnr {before.psnr:.2f} -> {after.psnr:.2f} dB, ssim {before.ssim:.4f} -> {after.ssim:.4f}")
