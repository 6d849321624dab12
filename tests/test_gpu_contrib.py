"""-m gpu: the contribution pass (m2s_contrib_begin / m2s_contrib_accumulate, k_splat_contrib) through the C ABI against the numpy
restatement tests/contrib_ref.py.  Pixel-centre Gaussians (g = exp(0) = 1 whatever exp is used) pin the weights exactly; elsewhere
the device's fast exp may move a weight — and a destination byte, hence later weights by one quantisation step — within
contrib_ref.W_BAR, and a count only for fragments whose weight lies within that bar of the threshold."""
import ctypes as C
import functools

import numpy as np
import pytest

import contrib_ref as cr
import splat_ref as sr
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.splat import SplatParams, to_c

pytestmark = pytest.mark.gpu
CW = 1.0 / 255.0
INVALID = 1


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def load(conv, quads, sources=None, n_records=None):
    q = np.ascontiguousarray(quads, np.float32).reshape(-1, 24)
    src = np.arange(q.shape[0], dtype=np.uint32) if sources is None else np.asarray(sources, np.uint32)
    n_records = int(n_records if n_records is not None else q.shape[0])
    conv.upload_records(np.zeros((n_records, 24), np.float32))
    conv.upload_quads(q)
    conv.upload_quad_sources(src)
    return src, n_records


def run(conv, quads, W, H, mode=0, cw=CW, sources=None, n_records=None):
    load(conv, quads, sources, n_records)
    conv.contrib_begin()
    conv.contrib_accumulate(SplatParams((W, H), mode), cw)
    w, n = conv.download_contrib()
    return w.view(np.uint32), n


@functools.lru_cache(maxsize=None)
def random_case(W, H, n, seed):
    q = sr.random_quads(n, W, H, seed, max_px=24.0)
    return q, cr.contrib(q, W, H, CW, cr.W_BAR)


def assert_within_bars(got_w, got_n, ref, what):
    dw = np.abs(got_w.view(np.float32).astype(np.float64) - ref["wmax"].view(np.float32).astype(np.float64))
    exact = float((got_w == ref["wmax"]).mean())
    print(f"{what}: max |d wmax| = {dw.max(initial=0.0):.3g} (bit-identical: {exact:.4f}), npix differs from the restatement's own count "
          f"at {int((got_n != ref['n']).sum())} of {got_n.size} (max |d npix| = {int(np.abs(got_n.astype(np.int64) - ref['n']).max(initial=0))}), "
          f"outside [n_lo, n_hi] at {int(((got_n < ref['n_lo']) | (got_n > ref['n_hi'])).sum())}")
    assert dw.max(initial=0.0) <= cr.W_BAR, what
    assert dw.max(initial=0.0) <= cr.W_GUARD, f"{what}: within the bar but beyond 4 x the achieved error"
    assert ((ref["n_lo"] <= got_n) & (got_n <= ref["n_hi"])).all(), what


# ---- exact: every quad covers the one pixel its mean sits on -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 5])
def test_pixel_centre_stacks_exact(conv, mode):
    W, H = 64, 32
    stacks = [[0.75], [0.5, 0.5], [0.3, 0.9, 0.2], [1.0, 0.8, 0.6, 0.4], [0.1, 0.2, 0.3, 0.4, 0.5], [0.9, 0.9, 0.9, 0.9, 0.9, 0.9]]
    qs, first = [], []
    for k, st in enumerate(stacks):
        first.append(len(qs))
        qs += [sr.quad_at(W, H, 3 + 6 * k, 2 + 3 * k, 0.6, a=a) for a in st]
    q = np.stack(qs)
    ref = cr.contrib(q, W, H, CW)
    assert np.array_equal(ref["n_lo"], ref["n_hi"])
    w, n = run(conv, q, W, H, mode)
    assert np.array_equal(w, ref["wmax"]) and np.array_equal(n, ref["n_lo"])
    # behind the quad with a = 1.0 nothing is left
    k = first[3]
    assert w[k] == np.float32(1.0).view(np.uint32) and n[k] == 1
    assert not w[k + 1:k + 4].any() and not n[k + 1:k + 4].any()
    # 0.9 six times: the pixel saturates on the way and the tail gets exactly 0
    assert w[first[5]] == np.float32(0.9).view(np.uint32) and w[first[5] + 5] == 0 and n[first[5] + 5] == 0


# ---- random overlapping quads: partial tiles, many tiles ----------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n,seed", [(64, 48, 500, 3), (641, 359, 3000, 1)])
def test_random_quads_within_bars(conv, W, H, n, seed):
    q, ref = random_case(W, H, n, seed)
    w, k = run(conv, q, W, H)
    assert_within_bars(w, k, ref, f"random {W}x{H}")
    assert (k > 0).sum() > n // 4


def test_one_tile_many_batches_opaque_layer(conv):
    """700 quads on one 16 x 16 tile = three LDS batches; quad 350 is an opaque layer over the whole tile: the workgroup's exit crosses
    the batch boundary and everything behind the layer is exactly 0."""
    W = H = 16
    q = sr.random_quads(700, W, H, 11, max_px=8.0, opacity=(0.004, 0.02))
    layer = sr.quad_at(W, H, 8, 8, 12.0, a=1.0, conic=(0.0, 0.0, 0.0))
    q[350] = layer
    ref = cr.contrib(q, W, H, CW, cr.W_BAR)
    assert ref["alpha"].min() == 255 and np.count_nonzero(ref["wmax"][:350]) > 300 and ref["n_lo"][350] == 256   # (the layer is not reached early)
    w, k = run(conv, q, W, H)
    assert not w[351:].any() and not k[351:].any()
    assert not ref["wmax"][351:].any()
    assert k[350] == 256 and w[350].view(np.float32) > 0.2
    assert_within_bars(w, k, ref, "one tile, three batches")


def test_one_quad_over_many_tiles(conv):
    """One quad over 13 x 13 tiles under smaller ones: its npix is the sum and its wmax the maximum over the tiles."""
    W = H = 256
    q = sr.random_quads(200, W, H, 5, max_px=20.0, opacity=(0.05, 0.4))
    big = sr.quad_at(W, H, 128, 128, 100.0, a=0.7, conic=(1e-4, 0.0, 1e-4))
    q = np.concatenate([q, big[None]])
    s = sr.setup(q, W, H)
    assert sr.tile_counts(s).sum() - sr.tile_counts(sr.setup(q[:-1], W, H)).sum() >= 100
    ref = cr.contrib(q, W, H, CW, cr.W_BAR, s=s)
    w, k = run(conv, q, W, H)
    assert_within_bars(w, k, ref, "one quad over 169 tiles")
    assert k[-1] > 20000


def test_sources_fold_quads_onto_records(conv):
    W, H, n, seed = 64, 48, 500, 3
    q, ref = random_case(W, H, n, seed)
    rng = np.random.default_rng(9)
    n_records = 640
    src = rng.permutation(n_records)[:n].astype(np.uint32)
    src[1] = src[0]                                       # two quads of one record
    src[77] = src[401]
    want = cr.per_record(ref, src, n_records)
    w, k = run(conv, q, W, H, sources=src, n_records=n_records)
    assert w.size == n_records
    assert_within_bars(w, k, want, "sources")
    untouched = np.setdiff1d(np.arange(n_records), src)
    assert untouched.size >= 140 and not w[untouched].any() and not k[untouched].any()


def test_skipped_quads_contribute_nothing(conv):
    W, H = 128, 96
    q = sr.random_quads(400, W, H, 7)
    q[5, 13] = np.nan
    q[17, 0] = np.inf
    q[33, 4] = 1e5                                        # beyond the guard band
    q[40, 22] = -np.inf
    s = sr.setup(q, W, H)
    assert s["skip"].sum() == 4
    ref = cr.contrib(q, W, H, CW, cr.W_BAR, s=s)
    w, k = run(conv, q, W, H)
    for i in (5, 17, 33, 40):
        assert w[i] == 0 and k[i] == 0
    assert_within_bars(w, k, ref, "skips")


def test_two_views_accumulate_max_and_sum(conv):
    W, H = 96, 64
    qa = sr.random_quads(300, W, H, 21)
    qb = sr.random_quads(260, W, H, 22)
    n_records = 320
    rng = np.random.default_rng(2)
    sa = rng.permutation(n_records)[:300].astype(np.uint32)
    sb = rng.permutation(n_records)[:260].astype(np.uint32)
    wa, ka = run(conv, qa, W, H, sources=sa, n_records=n_records)
    wb, kb = run(conv, qb, W, H, sources=sb, n_records=n_records)
    # both views into one pair of accumulators: the records stay, the quads change
    load(conv, qa, sa, n_records)
    conv.contrib_begin()
    conv.contrib_accumulate(SplatParams((W, H), 0), CW)
    conv.upload_quads(qb)
    conv.upload_quad_sources(sb)
    conv.contrib_accumulate(SplatParams((W, H), 0), CW)
    w, k = conv.download_contrib()
    assert np.array_equal(w.view(np.uint32), np.maximum(wa, wb)) and np.array_equal(k, ka + kb)
    # ... and a second run gives the same bits
    w2, k2 = run(conv, qa, W, H, sources=sa, n_records=n_records)
    assert np.array_equal(w2, wa) and np.array_equal(k2, ka)


def test_errors(conv, hiplib):
    W, H = 32, 32
    q = sr.random_quads(20, W, H, 1)
    h = conv._h

    def acc(mode=0, cw=CW, res=(W, H)):
        pc = to_c(SplatParams(res, mode))
        return hiplib.m2s_contrib_accumulate(h, C.byref(pc), C.c_float(cw))

    load(conv, q)
    conv.contrib_begin()
    assert acc() == 0
    assert acc(mode=4) == INVALID
    assert acc(mode=7) == INVALID
    for cw in (-1e-3, float("nan"), float("inf")):
        assert acc(cw=cw) == INVALID
    for res in ((0, 32), (32, 8193)):
        assert acc(res=res) == INVALID
    # sources missing: another producer of sorted quads
    conv.upload_quads(q)
    assert hiplib.m2s_device_sorted_sources(h) is None
    assert acc() == INVALID
    # a source beyond the records is refused at the door
    bad = np.arange(20, dtype=np.uint32)
    bad[3] = 20
    assert hiplib.m2s_upload_quad_sources(h, bad.ctypes.data, 20) == INVALID
    assert hiplib.m2s_upload_quad_sources(h, bad.ctypes.data, 19) == INVALID
    # records that changed since begin
    load(conv, q)
    assert acc() == INVALID
    assert hiplib.m2s_device_contrib(h, 0) is None
    # no begin at all
    c2 = Converter(0)
    try:
        c2.upload_records(np.zeros((20, 24), np.float32))
        c2.upload_quads(q)
        c2.upload_quad_sources(np.arange(20, dtype=np.uint32))
        pc = to_c(SplatParams((W, H), 0))
        assert hiplib.m2s_contrib_accumulate(c2._h, C.byref(pc), C.c_float(CW)) == INVALID
    finally:
        c2.close()
