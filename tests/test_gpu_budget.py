"""-m gpu: m2s_prune_budget / Converter.prune_budget against the numpy restatement (tests/budget_ref.py): crafted accumulators round
the wave and workgroup edges in every key family, the baked plane, thresholds together with a budget, m2s_prune when the budget does not
bind, the occlusion of one wall by another end to end, the AREA importance on planted records (uploaded and adopted), the error paths;
and, printed without an assertion, what a budget buys over truncation on two nested spheres."""
import ctypes as C

import numpy as np
import pytest

import budget_cases as bc
import budget_ref as br
import contrib_ref as cr
import prune_cases as pc
from mesh2splat_amd import synth
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prune import BudgetParamsC, orbit_cameras
from mesh2splat_amd.scene import Mesh, Scene
from mesh2splat_amd.splat import SplatParams

pytestmark = pytest.mark.gpu
PASS_ALL = (-1.0, 0)        # min_weight, min_pixels: every record is a candidate


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def crafted(conv, rec, w, k):
    conv.upload_records(rec)
    conv.contrib_begin()
    conv.upload_contrib(w, k)


def check_views(conv, rec, w, k, B, min_weight, min_pixels):
    kept, want = br.select(br.keys_views(w, k), br.candidates_views(w, k, min_weight, min_pixels), B)
    got = conv.prune_budget(B, "views", min_weight, min_pixels)
    assert got == want, (got, want)
    assert conv.num_stored == min(B, want["candidates"]) == kept.size
    assert np.array_equal(conv.download().view(np.uint32), rec[kept].view(np.uint32))
    return kept


@pytest.mark.parametrize("n", bc.SIZES)
@pytest.mark.parametrize("name", bc.FAMILIES)
def test_crafted_accumulators(conv, name, n):
    rec = bc.records(n, n)
    w, k = bc.family(name, n)
    for B in bc.budgets(n):
        crafted(conv, rec, w, k)
        back_w, back_k = conv.download_contrib()
        assert np.array_equal(back_w.view(np.uint32), w) and np.array_equal(back_k, k)
        check_views(conv, rec, w, k, B, *PASS_ALL)


def test_more_than_one_trip_of_the_grid_stride_kernels(conv):
    """The key and histogram kernels run at most 512 workgroups: past 131 072 records the first, past 524 288 the second goes round its
    loop more than once.  530 003 records (three keys behind the last group of four), random keys, then all ties."""
    n = 530003
    rec = np.zeros((n, 24), np.float32)
    rec[:, 0] = np.arange(n, dtype=np.float32)                                  # (exact below 2^24: the row says where it came from)
    for name, B in (("random", 200001), ("all_equal", 262145)):
        w, k = bc.family(name, n)
        crafted(conv, rec, w, k)
        check_views(conv, rec, w, k, B, *PASS_ALL)


def test_upload_contrib_leaves_a_null_accumulator_alone(conv):
    rec = bc.records(100, 1)
    w, k = bc.family("random", 100)
    crafted(conv, rec, w, None)
    assert not conv.download_contrib()[1].any()
    conv.upload_contrib(None, k)
    back_w, back_k = conv.download_contrib()
    assert np.array_equal(back_w.view(np.uint32), w) and np.array_equal(back_k, k)
    conv.upload_contrib(w.view(np.float32), None)                               # the weights themselves are taken as their bits
    assert np.array_equal(conv.download_contrib()[0].view(np.uint32), w)
    half = np.full(100, 0.5)                                                    # float64 weights are rounded to float32, never truncated to 0
    conv.upload_contrib(half, None)
    assert (conv.download_contrib()[0].view(np.uint32) == 0x3F000000).all()
    for bad_w, bad_k in ((k.astype(np.int64), None), (None, k.astype(np.float32)), (None, k.astype(np.uint64)), (w.astype(np.int32), None)):
        with pytest.raises(TypeError):
            conv.upload_contrib(bad_w, bad_k)
    assert (conv.download_contrib()[0].view(np.uint32) == 0x3F000000).all() and np.array_equal(conv.download_contrib()[1], k)


def test_sh_plane_is_compacted_alongside(conv):
    n, B = 256, 100
    rec = np.ascontiguousarray(synth_records(n))
    conv.upload_records(rec)
    sh = conv.bake_light(BakeParams(n_theta=4, n_phi=8, use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)))
    assert sh.shape == (n, 48) and np.unique(sh[:, 0]).size > n // 2
    w, k = bc.family("random", n)
    conv.contrib_begin()
    conv.upload_contrib(w, k)
    kept = check_views(conv, rec, w, k, B, *PASS_ALL)
    assert np.array_equal(conv.download_sh().view(np.uint32), sh[kept].view(np.uint32))


def synth_records(n):
    """records a bake has something to say about: unit normals, positions round the origin, colours and pbr in [0, 1]"""
    import compact_ref
    return compact_ref.make_records(n, 21)


def test_thresholds_and_budget_together(conv):
    n = 1000
    rec = bc.records(n, 2)
    w, k = bc.family("random", n)
    tau = float(np.median(w.view(np.float32)))
    nc = int(br.candidates_views(w, k, tau, 3).sum())
    assert 100 < nc < n - 100
    for B in (1, nc // 3, nc - 1):
        crafted(conv, rec, w, k)
        check_views(conv, rec, w, k, B, tau, 3)


def test_equals_prune_when_the_budget_does_not_bind(hiplib, conv):
    n = 1000
    rec = bc.records(n, 3)
    w, k = bc.family("half_zero", n)
    tau = float(np.median(w.view(np.float32)))
    other = Converter(0)
    try:
        for B in (n, n + 5, 1 << 40):
            crafted(conv, rec, w, k)
            crafted(other, rec, w, k)
            pruned = other.prune(tau, 2)
            got = conv.prune_budget(B, "views", tau, 2)
            assert got["kept"] == got["candidates"] == pruned["kept"] == conv.num_stored == other.num_stored and 0 < got["kept"] < n
            assert (got["threshold_key"], got["ties_kept"], got["ties"]) == (0, 0, 0)
            assert np.array_equal(conv.download().view(np.uint32), other.download().view(np.uint32))
    finally:
        other.close()


def test_occlusion_keeps_exactly_the_front_wall(conv, oracle):
    """prune_cases.two_walls through wall_params(): every back-wall record has wmax = 0, hence key 0; every front-wall record has
    wmax >= 0.1506 > 1 / 255, hence npix >= 1 and key > 0.  FIRST the restatement alone — contrib_ref on the oracle's
    prepass, then budget_ref, with either end of the restatement's npix interval — THEN the device chain m2s_prepass_sorted ->
    m2s_contrib_accumulate -> m2s_prune_budget(1024, VIEWS): the front wall, byte for byte."""
    CW = 1.0 / 255.0
    W, H = pc.WALL_SIZE
    conv.upload_scene(pc.two_walls())
    n = conv.convert(pc.WALL_R)
    rec = conv.download()
    front = rec[:, 2] > 0
    B = int(front.sum())
    assert B == 1024 and n == 1024 + 26 * 26
    p = pc.wall_params()
    quads, src = pc.sorted_with_sources(oracle, p, rec)
    ref = cr.per_record(cr.contrib(quads, W, H, CW, cr.W_BAR), src, n)
    everyone = np.ones(n, bool)
    for npix in (ref["n_lo"], ref["n_hi"]):
        keys = br.keys_views(ref["wmax"], npix)
        assert not keys[~front].any() and keys[front].min() > 0
        kept, counts = br.select(keys, everyone, B)
        assert np.array_equal(kept, np.flatnonzero(front)) and counts["threshold_key"] > 0
    # the device
    conv.contrib_begin()
    assert conv.prepass_sorted(p, download=False) == n
    conv.contrib_accumulate(SplatParams((W, H), 0), CW)
    w, k = conv.download_contrib()
    keys = br.keys_views(w.view(np.uint32), k)
    print(f"device: back wall max key = {keys[~front].max():#x}, front wall min key = {keys[front].min():#x}")
    got = conv.prune_budget(B, "views", *PASS_ALL)
    assert got == br.select(keys, everyone, B)[1] and got["kept"] == B
    assert np.array_equal(conv.download().view(np.uint32), rec[front].view(np.uint32))


def test_area_planted_records(conv):
    rec = bc.planted_area_records()
    kept, want = br.select(br.keys_area(rec), np.ones(len(rec), bool), 100)
    assert want["threshold_key"] > 0 and 40 in kept and 41 in kept and 90 in kept and 30 not in kept and 60 not in kept
    conv.upload_records(rec)
    assert conv.prune_budget(100, "area", float("nan"), 1 << 31) == want          # (AREA reads neither threshold)
    assert conv.num_stored == 100 and np.array_equal(conv.download().view(np.uint32), rec[kept].view(np.uint32))
    # again on the survivors (records already pruned), into all ties: key 0 for everyone
    zero = rec.copy()
    zero[:, 7] = 0
    conv.upload_records(zero)
    got = conv.prune_budget(7, "area")
    assert got == dict(zip(br.COUNTS, (len(rec), len(rec), 7, 0, 7, len(rec))))
    assert np.array_equal(conv.download().view(np.uint32), zero[:7].view(np.uint32))


def test_area_adopted_records_go_into_the_pool(conv):
    rec = bc.planted_area_records()
    kept, want = br.select(br.keys_area(rec), np.ones(len(rec), bool), 100)
    owner = Converter(0)                                                                     # the "caller": its buffer is not conv's
    try:
        owner.upload_records(rec)
        mine = owner.device_records
        conv.set_records(mine, len(rec), 32)
        assert conv.device_records == mine
        assert conv.prune_budget(100, "area") == want
        assert conv.device_records not in (0, mine)
        assert np.array_equal(owner.download().view(np.uint32), rec.view(np.uint32))          # the caller's memory is not written
        assert np.array_equal(conv.download().view(np.uint32), rec[kept].view(np.uint32))
        got = conv.prune_budget(40, "area")                                                  # the survivors live in the pool now
        kept2, want2 = br.select(br.keys_area(rec[kept]), np.ones(100, bool), 40)
        assert got == want2 and np.array_equal(conv.download().view(np.uint32), rec[kept][kept2].view(np.uint32))
    finally:
        owner.close()


def test_errors(hiplib):
    c = Converter(0)
    try:
        def call(max_records=1, importance=0, min_weight=0.0, reserved=0):
            bp = BudgetParamsC(max_records, min_weight, 0, importance, reserved)
            return hiplib.m2s_prune_budget(c._h, C.byref(bp), None)
        assert call(importance=1) == 7 and call() == 7                              # no records at all
        rec = bc.records(50, 4)
        c.upload_records(rec)
        assert call(max_records=0, importance=1) == 1 and call(importance=1, reserved=1) == 1 and call(importance=2) == 1
        assert call() == 7                                                          # VIEWS without accumulators
        c.contrib_begin()
        assert call(min_weight=float("nan")) == 1 and call(max_records=0) == 1
        assert hiplib.m2s_prune_budget(c._h, None, None) == 1
        w = np.zeros(50, np.uint32)
        assert hiplib.m2s_upload_contrib(c._h, w.ctypes.data, None, 49) == 1         # another n
        w[7] = bc.ONE + 1
        assert hiplib.m2s_upload_contrib(c._h, w.ctypes.data, None, 50) == 1         # not the bits of a weight in [0, 1]
        w[7] = bc.ONE
        assert hiplib.m2s_upload_contrib(c._h, w.ctypes.data, None, 50) == 0
        assert c.num_stored == 50 and np.array_equal(c.download().view(np.uint32), rec.view(np.uint32))     # nothing above touched the records
        assert call(max_records=10, min_weight=-1.0) == 0 and c.num_stored == 10
        assert call(max_records=5, min_weight=-1.0) == 7                            # the accumulators went with the old records
        assert hiplib.m2s_upload_contrib(c._h, w.ctypes.data, None, 10) == 7
        with pytest.raises(M2SError):
            c.prune_budget(5, "views")
        with pytest.raises(KeyError):
            c.prune_budget(5, "volume")
        assert c.prune_budget(5, "area")["kept"] == 5
        # conversions in flight: refused for either importance, nothing touched, the conversion still delivered
        c.upload_scene(synth.cube_sphere(6, tex_size=16))
        c.submit(48)
        total = c.wait()                                                            # (the first conversion of a scene runs inside submit)
        before = c.download()
        assert total > 100 and c.num_stored == len(before)
        c.contrib_begin()                                                           # valid accumulators: VIEWS has nothing else to object to
        c.submit(48)
        for importance in (0, 1):
            assert call(max_records=10, importance=importance, min_weight=-1.0) == 7
            assert b"in flight" in hiplib.m2s_last_error(c._h)
        assert c.wait() == total and c.num_stored == len(before)
        assert np.array_equal(c.download().view(np.uint32), before.view(np.uint32))
        assert c.prune_budget(10, "area")["kept"] == 10                             # ... and once it has been waited for, the call goes through
    finally:
        c.close()


def test_nested_spheres_budget_against_truncation(conv):
    """What the budget buys over the cap on one scene (tests/test_gpu_prune.py's nested spheres, R = 64, 128 x 128, three views at 20
    degrees): PSNR / SSIM with every record, with half of them chosen by VIEWS, by AREA, and with the first half (what a cap keeps).
    Printed, not asserted."""
    R, W, H = 64, 128, 128
    scene = Scene([Mesh(name="outer", vertices=synth.cube_sphere_vertices(10, 1.0), base_color=(0.8, 0.6, 0.4, 1.0)),
                   Mesh(name="inner", vertices=synth.cube_sphere_vertices(8, 0.5), base_color=(0.2, 0.4, 0.9, 1.0))])
    light = (2.0, 2.5, 3.0)
    score_cams = orbit_cameras(scene, 3, W, H, (20.0,))
    conv.upload_scene(scene)
    n = conv.convert(R)
    B = n // 2
    rec = conv.download()

    def score():
        return conv.score_views(score_cams, R, light, 30.0, shadow_resolution=128)[1]

    out = {"all": (n, score())}
    counts = conv.prune_views(orbit_cameras(scene, 6, 2 * W, 2 * H, (-30.0, 30.0)), R, (W, H), budget=B)
    assert counts["before"] == n and counts["kept"] == conv.num_stored == min(B, counts["candidates"])
    out["views"] = (counts["kept"], score())
    assert conv.convert(R) == n
    counts = conv.prune_budget(B, "area")
    assert counts["kept"] == conv.num_stored == B
    out["area"] = (B, score())
    conv.set_max_gaussians(B)
    try:
        assert conv.convert(R) == n and conv.num_stored == B
        assert np.array_equal(conv.download().view(np.uint32), rec[:B].view(np.uint32))
        out["cap"] = (B, score())
    finally:
        conv.set_max_gaussians(-1)
    for name, (m, s) in out.items():
        print(f"nested spheres, {name}: {m} records, psnr {s.psnr:.2f} dB, ssim {s.ssim:.4f}")
