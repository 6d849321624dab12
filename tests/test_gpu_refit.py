"""-m gpu: the colour refit (m2s_refit_begin / _accumulate / _apply, k_splat_refit, k_refit_apply) through the C ABI against the numpy
restatement tests/refit_ref.py.  Pixel-centre Gaussians (g = exp(0) = 1 whatever exp is used) pin the accumulators exactly; elsewhere
the device's fast exp may move a weight — and a destination byte, hence later weights by one quantisation step — within
contrib_ref.W_BAR per fragment, which refit_ref.WQ_BAR carries over to the integer sums.  The apply is exact everywhere."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import refit_ref as rr
import splat_ref as sr
from mesh2splat_amd import _lib, gltf_io, synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.prune import orbit_cameras
from mesh2splat_amd.refit import RefitApplyParamsC, RefitParams, RefitParamsC, to_c
from mesh2splat_amd.scene import Mesh, Scene

pytestmark = pytest.mark.gpu
INVALID, STATE = 1, 7
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "mesh2splat")


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def random_planes(W, H, seed, target_alpha=255, render_alpha=(100, 256)):
    """Two (H, W, 4) uint8 planes: a covered target and a render whose alpha straddles min_cover = 128, colours up to the alpha."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    t[..., 3] = target_alpha
    r = np.zeros((H, W, 4), np.uint8)
    r[..., 3] = rng.integers(render_alpha[0], render_alpha[1], (H, W))
    r[..., :3] = (rng.random((H, W, 3)) * (r[..., 3:4].astype(np.float64) + 1.0)).astype(np.uint8)
    return t, r


def load(conv, quads, sources=None, n_records=None):
    q = np.ascontiguousarray(quads, np.float32).reshape(-1, 24)
    src = np.arange(q.shape[0], dtype=np.uint32) if sources is None else np.asarray(sources, np.uint32)
    n_records = int(n_records if n_records is not None else q.shape[0])
    conv.upload_records(np.zeros((n_records, 24), np.float32))
    conv.upload_quads(q)
    conv.upload_quad_sources(src)
    return src, n_records


def run(conv, quads, W, H, target, render, min_cover=128, sources=None, n_records=None):
    import torch
    load(conv, quads, sources, n_records)
    conv.refit_begin()
    counts = conv.refit_accumulate(RefitParams((W, H), min_cover), torch.from_numpy(target).cuda(), torch.from_numpy(render).cuda())
    num, den = conv.download_refit()
    return num, den, counts


@functools.lru_cache(maxsize=None)
def random_case(W, H, n, seed):
    q = sr.random_quads(n, W, H, seed, max_px=24.0)
    t, r = random_planes(W, H, seed + 100)
    return q, t, r, rr.accumulate(q, np.arange(n), n, W, H, t, r, 128)


# ---- exact: every quad covers the one pixel its mean sits on -----------------------------------------------------------------------
def test_pixel_centre_stacks_exact(conv):
    W, H = 64, 32
    stacks = [[0.75], [0.5, 0.5], [0.3, 0.9, 0.2], [1.0, 0.8, 0.6, 0.4], [0.1, 0.2, 0.3, 0.4, 0.5], [0.9, 0.9, 0.9, 0.9, 0.9, 0.9]]
    qs, first = [], []
    for k, st in enumerate(stacks):
        first.append(len(qs))
        qs += [sr.quad_at(W, H, 3 + 6 * k, 2 + 3 * k, 0.6, a=a) for a in st]
    q = np.stack(qs)
    t, r = random_planes(W, H, 7, render_alpha=(128, 256))
    ref = rr.accumulate(q, np.arange(len(qs)), len(qs), W, H, t, r, 128)
    num, den, counts = run(conv, q, W, H, t, r)
    assert np.array_equal(num, ref["num"]) and np.array_equal(den, ref["den"])
    assert counts == {"pixels": W * H, "pairs": ref["pairs"]}
    # behind the quad with a = 1.0 nothing is left; 0.9 six times saturates on the way
    k = first[3]
    assert den[k] == 65536 and not den[k + 1:k + 4].any() and not num[k + 1:k + 4].any()
    assert den[first[5]] == np.rint(np.float32(0.9) * np.float32(65536)) and den[first[5] + 5] == 0
    assert np.count_nonzero(num) > 20


# ---- random overlapping quads: partial tiles, several tiles -------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n,seed", [(64, 48, 500, 3), (41, 23, 200, 5)])
def test_random_quads_within_bars(conv, W, H, n, seed):
    q, t, r, ref = random_case(W, H, n, seed)
    num, den, counts = run(conv, q, W, H, t, r)
    rr.assert_within_bars(num, den, ref, f"random {W}x{H}")
    assert counts == {"pixels": ref["pixels"], "pairs": ref["pairs"]} and 0 < ref["pixels"] < W * H
    assert (den > 0).sum() > n // 4 and np.count_nonzero(num) > n // 4


def test_two_runs_give_identical_words(conv):
    W, H, n, seed = 64, 48, 500, 3
    q, t, r, _ = random_case(W, H, n, seed)
    a = run(conv, q, W, H, t, r)
    b = run(conv, q, W, H, t, r)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_one_tile_many_batches_opaque_layer(conv):
    """700 quads on one 16 x 16 tile = three LDS batches; quad 350 is an opaque layer over the whole tile: the workgroup's exit crosses
    the batch boundary and every accumulator behind the layer is exactly 0."""
    W = H = 16
    q = sr.random_quads(700, W, H, 11, max_px=8.0, opacity=(0.004, 0.02))
    q[350] = sr.quad_at(W, H, 8, 8, 12.0, a=1.0, conic=(0.0, 0.0, 0.0))
    t, r = random_planes(W, H, 12, render_alpha=(128, 256))
    ref = rr.accumulate(q, np.arange(700), 700, W, H, t, r, 128)
    assert np.count_nonzero(ref["den"][:350]) > 300 and ref["den"][350] > 256 * 10000 and not ref["den"][351:].any()
    num, den, _ = run(conv, q, W, H, t, r)
    assert not den[351:].any() and not num[351:].any()
    rr.assert_within_bars(num, den, ref, "one tile, three batches")


def test_sums_fold_across_tiles_and_quads(conv):
    """One quad over 8 x 8 tiles under smaller ones, and two quads made from one record: a record's words are the sums over the tiles
    and over its quads."""
    W = H = 128
    q = sr.random_quads(150, W, H, 5, max_px=20.0, opacity=(0.05, 0.4))
    big = sr.quad_at(W, H, 64, 64, 60.0, a=0.7, conic=(1e-4, 0.0, 1e-4))
    q = np.concatenate([q, big[None]])
    n = q.shape[0]
    n_records = 200
    src = np.random.default_rng(9).permutation(n_records)[:n].astype(np.uint32)
    src[1] = src[0]
    src[77] = src[101]
    t, r = random_planes(W, H, 6)
    s = sr.setup(q, W, H)
    assert sr.tile_counts(s).sum() - sr.tile_counts(sr.setup(q[:-1], W, H)).sum() >= 49
    ref = rr.accumulate(q, src, n_records, W, H, t, r, 128, s=s)
    num, den, counts = run(conv, q, W, H, t, r, sources=src, n_records=n_records)
    assert den.size == n_records and counts["pairs"] == ref["pairs"]
    rr.assert_within_bars(num, den, ref, "one quad over 64 tiles, shared sources")
    assert den[src[-1]] > 65536 * 1000
    untouched = np.setdiff1d(np.arange(n_records), src)
    assert untouched.size >= 49 and not den[untouched].any() and not num[untouched].any()


def test_masked_pixels_add_nothing(conv):
    """Target alpha 0 on the left half, render alpha below min_cover on a band, and a block with sa = 1, s = 255 (the clamp)."""
    W, H, n, seed = 64, 48, 500, 3
    q = random_case(W, H, n, seed)[0]
    t, r = random_planes(W, H, 31, render_alpha=(200, 256))
    t[:, :W // 2, 3] = 0
    r[10:20, :, 3] = 127
    r[30:40, 40:60] = (255, 255, 255, 1)
    ref = rr.accumulate(q, np.arange(n), n, W, H, t, r, 128)
    num, den, counts = run(conv, q, W, H, t, r)
    assert counts["pixels"] == ref["pixels"] == (W // 2) * (H - 10) - 10 * 20
    rr.assert_within_bars(num, den, ref, "masked")
    # min_cover = 1 lets the block in: every error there is the clamp's -4096
    ref1 = rr.accumulate(q, np.arange(n), n, W, H, t, r, 1)
    num1, den1, counts1 = run(conv, q, W, H, t, r, min_cover=1)
    assert counts1["pixels"] == ref1["pixels"] == (W // 2) * H
    rr.assert_within_bars(num1, den1, ref1, "masked, min_cover 1")
    assert (rr.participation(t, r, 1)[1].reshape(H, W, 3)[30:40, 40:60] == -4096).all() and (num1 < 0).any()
    # an all-masked view adds exactly nothing
    t[..., 3] = 0
    num0, den0, counts0 = run(conv, q, W, H, t, r)
    assert counts0["pixels"] == 0 and not num0.any() and not den0.any()


def test_quads_outside_the_view_leave_only_the_pixel_count(conv):
    """No (tile, quad) pair at all: the kernel still counts the participating pixels and adds nothing."""
    W, H = 41, 23
    q = sr.random_quads(30, W, H, 8, max_px=4.0)
    q[:, 0] += 5.0                                           # (far to the right of the viewport, inside the guard band)
    t, r = random_planes(W, H, 9)
    ref = rr.accumulate(q, np.arange(30), 30, W, H, t, r, 128)
    assert ref["pairs"] == 0 and not ref["den"].any()
    num, den, counts = run(conv, q, W, H, t, r)
    assert counts == {"pixels": ref["pixels"], "pairs": 0} and counts["pixels"] > 0 and not num.any() and not den.any()


def test_two_views_add_up(conv):
    import torch
    W, H = 64, 48
    qa, ta, ra, _ = random_case(W, H, 500, 3)
    qb = sr.random_quads(300, W, H, 22)
    tb, rb = random_planes(W, H, 23)
    sb = np.random.default_rng(2).permutation(500)[:300].astype(np.uint32)
    na, da, _ = run(conv, qa, W, H, ta, ra)
    nb, db, _ = run(conv, qb, W, H, tb, rb, sources=sb, n_records=500)
    load(conv, qa)
    conv.refit_begin()
    conv.refit_accumulate(RefitParams((W, H), 128), torch.from_numpy(ta).cuda(), torch.from_numpy(ra).cuda())
    conv.upload_quads(qb)
    conv.upload_quad_sources(sb)
    conv.refit_accumulate(RefitParams((W, H), 128), torch.from_numpy(tb).cuda(), torch.from_numpy(rb).cuda())
    num, den = conv.download_refit()
    assert np.array_equal(num, na + nb) and np.array_equal(den, da + db)


# ---- the apply, exact ---------------------------------------------------------------------------------------------------------------
def crafted(n=300, seed=4):
    rng = np.random.default_rng(seed)
    rec = rng.uniform(-2, 2, (n, 24)).astype(np.float32)
    rec[:, 4:8] = rng.uniform(0, 1, (n, 4)).astype(np.float32)
    den = rng.integers(1, 1 << 45, n, dtype=np.uint64)
    num = (rng.uniform(-1, 1, (n, 3)) * den[:, None].astype(np.float64) * 4096.0).astype(np.int64)
    one = 65536
    den[0], num[0] = 4 * one, (-4 * one * 2048, 4 * one * 4096, -4 * one * 4096)      # a negative num; both clamps at step 0.5 from (0.9, 0.9, 0.1)
    rec[0, 4:7] = (0.9, 0.9, 0.1)
    den[1], den[2], den[3] = 3 * one - 1, 3 * one, 0                      # below the threshold 3.0, at it, no weight at all
    num[3] = (5, -5, 5)
    rec[4, 5] = np.nan                                                    # one channel is not finite: its neighbours still move
    rec[5, 4] = np.inf
    den[6], num[6] = (1 << 45) + 12345, (-(1 << 57) + 99, (1 << 57) - 77, 3)      # words near the bounds of the pin
    return rec, num, den


def test_apply_matches_the_restatement_byte_for_byte(conv):
    rec, num, den = crafted()
    want, want_counts = rr.apply(rec, num, den, 0.5, 3.0)
    conv.upload_records(rec)
    conv.refit_begin()
    conv.upload_refit(num, den)
    got_num, got_den = conv.download_refit()
    assert np.array_equal(got_num, num) and np.array_equal(got_den, den)
    counts = conv.refit_apply(0.5, 3.0)
    got = conv.download()
    assert counts == want_counts and counts["no_weight"] >= 2 and counts["clamped"] >= 1
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    diff = got.view(np.uint8).reshape(len(rec), 96) != rec.view(np.uint8).reshape(len(rec), 96)
    assert diff.any() and not diff[:, :16].any() and not diff[:, 28:].any()
    assert not diff[1].any() and diff[2].any() and not diff[3].any() and not diff[4, 20:24].any() and not diff[5, 16:20].any()
    assert got[0, 4:7].tolist() == [np.float32(np.float64(np.float32(0.9)) - 0.25), 1.0, 0.0]
    # step 0 leaves the bits of every finite channel in [0, 1]
    conv.upload_records(rec)
    conv.refit_begin()
    conv.upload_refit(num, den)
    conv.refit_apply(0.0, 0.0)
    assert np.array_equal(conv.download().view(np.uint32), rr.apply(rec, num, den, 0.0, 0.0)[0].view(np.uint32))


# ---- what the apply does to the context ---------------------------------------------------------------------------------------------
def test_apply_invalidates_what_was_derived_from_the_old_colours(conv, hiplib, tmp_path):
    import torch
    from mesh2splat_amd.bake import BakeParams
    from mesh2splat_amd.light import LightParams
    scene = Scene([Mesh(name="s", vertices=synth.cube_sphere_vertices(4, 1.0), base_color=(0.8, 0.6, 0.4, 1.0))])
    conv.upload_scene(scene)
    n = conv.convert(24)
    rec = conv.download()
    conv.bake_light(BakeParams(use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)), download=False)
    conv.export_ply_sh(str(tmp_path / "before.ply"))
    cam = orbit_cameras(scene, 1, 64, 48, (20.0,))[0]
    pp, _ = cam.frame_params(24, (0, 0, 0), 0.0)
    assert conv.prepass_sorted(pp, download=False) > 0 and conv.device_sorted_sources
    conv.contrib_begin()
    conv.refit_begin()
    num = np.zeros((n, 3), np.int64)
    num[:, 0] = 65536 * 409
    conv.upload_refit(num, np.full(n, 65536, np.uint64))
    assert conv.device_refit(0) and conv.device_refit(1)
    h = conv._h
    counts = conv.refit_apply(1.0, 1.0)
    assert counts == {"records": n, "updated": n, "clamped": int((rec[:, 4].astype(np.float64) + 409 / 4096.0 > 1).sum()), "no_weight": 0}
    assert conv.num_stored == n
    assert not conv.device_sorted_sources and not conv.device_refit(0) and not conv.device_contrib(0)
    buf = (C.c_uint64 * n)()
    assert hiplib.m2s_download_contrib(h, buf, None, n) == STATE
    assert hiplib.m2s_download_refit(h, None, buf, n) == STATE
    assert hiplib.m2s_export_ply_sh(h, str(tmp_path / "after.ply").encode(), C.c_float(0.65)) == STATE
    pa = RefitApplyParamsC(1.0, 1.0)
    assert hiplib.m2s_refit_apply(h, C.byref(pa), None) == STATE
    got = conv.download()
    assert np.array_equal(got.view(np.uint32), rr.apply(rec, num, np.full(n, 65536, np.uint64))[0].view(np.uint32))
    conv.export_ply(str(tmp_path / "plain.ply"))                                # (the resolutionTarget is kept)
    # adopted records are copied into the pool first: the caller's memory is not written
    mine = torch.from_numpy(rec.copy()).cuda()
    conv.set_records(mine.data_ptr(), n, 24)
    conv.refit_begin()
    conv.upload_refit(num, np.full(n, 65536, np.uint64))
    conv.refit_apply(1.0, 1.0)
    assert conv.device_records != mine.data_ptr()
    assert np.array_equal(mine.cpu().numpy().view(np.uint32), rec.view(np.uint32))
    assert np.array_equal(conv.download().view(np.uint32), got.view(np.uint32))


def test_errors(conv, hiplib):
    import torch
    W, H = 32, 32
    q = sr.random_quads(20, W, H, 1)
    t, r = (torch.from_numpy(p).cuda() for p in random_planes(W, H, 1))
    h = conv._h

    def acc(res=(W, H), min_cover=128, reserved=0, handle=None, target=t, render=r):
        pc = to_c(RefitParams(res, min_cover))
        pc.reserved = reserved
        return hiplib.m2s_refit_accumulate(handle or h, C.byref(pc), target.data_ptr() if target is not None else None,
                                           render.data_ptr() if render is not None else None, None)

    def app(step=1.0, mws=1.0, reserved=0, handle=None):
        pa = RefitApplyParamsC(step, mws)
        pa.reserved[1] = reserved
        return hiplib.m2s_refit_apply(handle or h, C.byref(pa), None)

    load(conv, q)
    conv.refit_begin()
    assert acc() == 0
    for mc in (0, 256):
        assert acc(min_cover=mc) == INVALID
    assert acc(reserved=1) == INVALID
    for res in ((0, 32), (32, 8193)):
        assert acc(res=res) == INVALID
    for bad in (dict(step=float("nan")), dict(step=float("inf")), dict(mws=-1.0), dict(mws=float("nan")), dict(mws=float("inf")), dict(reserved=1)):
        assert app(**bad) == INVALID
    # sources missing: another producer of sorted quads
    conv.upload_quads(q)
    assert acc() == INVALID
    # records that changed since begin
    load(conv, q)
    assert acc() == INVALID and app() == STATE
    assert hiplib.m2s_device_refit(h, 0) is None
    assert hiplib.m2s_upload_refit(h, None, None, 20) == STATE
    conv.refit_begin()
    assert hiplib.m2s_upload_refit(h, None, None, 19) == INVALID
    assert hiplib.m2s_download_refit(h, None, None, 19) == 5                     # M2S_ERR_CAPACITY
    # a fresh context: no records, no begin, no G-buffers behind a NULL plane
    c2 = Converter(0)
    try:
        assert hiplib.m2s_refit_begin(c2._h) == STATE
        c2.upload_records(np.zeros((20, 24), np.float32))
        c2.upload_quads(q)
        c2.upload_quad_sources(np.arange(20, dtype=np.uint32))
        assert acc(handle=c2._h) == INVALID and app(handle=c2._h) == STATE
        c2.refit_begin()
        assert acc(handle=c2._h, target=None) == STATE and acc(handle=c2._h, render=None) == STATE
        assert acc(handle=c2._h) == 0
    finally:
        c2.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def quad_scene():
    s = synth.unit_quad()
    s.meshes[0].base_color = (0.8, 0.4, 0.2, 1.0)
    return s


def test_refit_views_recovers_a_flat_colour(conv):
    """The unit quad with base colour (0.8, 0.4, 0.2), R = 32, one camera at 96 x 64 (raised by 20 degrees: seen exactly head-on flat
    isotropic Gaussians lose quads to NaN axes, tests/test_contrib_cpu.py); the records re-uploaded with colour 0.5."""
    scene = quad_scene()
    conv.upload_scene(scene)
    n = conv.convert(32)
    rec = conv.download()
    assert n > 500 and np.allclose(rec[:, 4:7], (0.8, 0.4, 0.2), atol=1e-6)
    grey = rec.copy()
    grey[:, 4:7] = 0.5
    conv.upload_records(grey)
    cams = orbit_cameras(scene, 1, 96, 64, (20.0,))
    out = conv.refit_views(cams, 32, iterations=2)
    print("refit_views:", out)
    assert out["iterations"] == 2 and out["views"] == 1 and len(out["sse"]) == 3 and out["pixels"][0] > 500
    assert out["updated"][0] > n // 2 and out["updated"][0] + out["no_weight"][0] == n
    assert out["sse"][0] > 0 and out["sse"][2] * 4 < out["sse"][0]
    got = conv.download()
    seen = np.abs(got[:, 4:7] - grey[:, 4:7]).max(1) > 0
    # every record that moved ended closer to the mesh colour than grey was, channel by channel (records at the rim overshoot a little:
    # their pixels are shared with neighbours that were as wrong as they were)
    err = np.abs(got[seen, 4:7] - np.float32((0.8, 0.4, 0.2)))
    print(f"updated records: max colour error {err.max(0)}, median {np.median(err, 0)}")
    assert seen.sum() > n // 2 and (err < np.abs(np.float32(0.5) - np.float32((0.8, 0.4, 0.2)))).all()
    assert np.array_equal(got[:, 7], rec[:, 7]) and np.array_equal(got[:, :4].view(np.uint32), rec[:, :4].view(np.uint32))


def test_cli_refit(tmp_path, hiplib):
    glb, out = str(tmp_path / "q.glb"), str(tmp_path / "q.ply")
    gltf_io.write_glb(quad_scene(), glb)
    base = [EXE, glb, out, "--density", "32", "--preview-size", "96x64"]
    r = subprocess.run(base + ["--refit", "1", "--refit-elevations", "20", "--refit-iters", "2", "--refit-step", "1"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("refit: ")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0][len("refit: "):])
    assert j["iterations"] == 2 and j["views"] == 1 and j["size"] == [96, 64] and j["density"] == 32 and j["step"] == 1.0
    assert len(j["sse"]) == 3 and len(j["updated"]) == 2 and len(j["clamped"]) == 2 and len(j["no_weight"]) == 2 and j["pixels"][0] > 500
    for bad in (["--refit", "0"], ["--refit", "1", "--refit-iters", "0"], ["--refit", "1", "--refit-step", "nan"], ["--refit", "1", "--refit-elevations", "90"],
                ["--refit", "1", "--gpus", "2"]):
        assert subprocess.run(base + bad, capture_output=True, text=True, timeout=300).returncode == 2, bad
