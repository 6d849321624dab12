"""The colour refit's restatement (tests/refit_ref.py) against hand-checked values, exact rational arithmetic and the property the
end-to-end GPU test rests on; and the sizes of the two parameter structs.  No GPU."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

import refit_ref as rr
import splat_ref as sr


def planes(W, H, target_rgba, render_rgba):
    t = np.zeros((H, W, 4), np.uint8)
    r = np.zeros((H, W, 4), np.uint8)
    t[:] = target_rgba
    r[:] = render_rgba
    return t, r


def test_hand_checked_one_fragment():
    W, H = 8, 8
    q = sr.quad_at(W, H, 3, 2, 0.6, a=1.0)[None]
    t, r = planes(W, H, (204, 204, 204, 255), (128, 128, 128, 255))
    ref = rr.accumulate(q, [0], 1, W, H, t, r, 128)
    # n = 4096 * 255 * 76, d = 255 * 255: 4096 * 76 / 255 = 1220.77 -> 1221; one fragment with w = 1 * (1 - 0) = 1
    assert ref["den"].tolist() == [65536] and ref["num"].tolist() == [[65536 * 1221] * 3]
    assert ref["frags"].tolist() == [1] and ref["pixels"] == W * H and ref["pairs"] == 1
    rec = np.zeros((1, 24), np.float32)
    rec[0, 4:8] = (0.5, 0.5, 0.5, 0.25)
    out, counts = rr.apply(rec, ref["num"], ref["den"], 1.0, 1.0)
    want = np.float32(0.5 + 1221 / 4096.0)
    assert out[0, 4:7].tolist() == [want] * 3 and out[0, 7] == np.float32(0.25)
    assert counts == dict(records=1, updated=1, clamped=0, no_weight=0)
    changed = np.nonzero(out.view(np.uint8)[0] != rec.view(np.uint8)[0])[0]
    assert changed.min() >= 16 and changed.max() <= 27


def test_error_rule_is_the_rounded_rational():
    """eq = round-half-up(4096 (m / 255 - s / sa)) clamped to +-4096, over every (m, s) for three sa — the clamp included."""
    for sa in (1, 128, 255):
        m, s = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
        got = rr.error_q(m, s, sa)
        want = np.empty((256, 256), np.int64)
        for a in range(256):
            for b in range(256):
                e = (Fraction(a, 255) - Fraction(b, sa)) * 4096 + Fraction(1, 2)
                want[a, b] = min(max(math.floor(e), -4096), 4096)
        assert np.array_equal(got, want), sa
        if sa == 1:
            assert got.min() == -4096 and (got == -4096).sum() > 60000          # (s > sa: the clamp does the work)
        else:
            assert got.max() == 4096 and got[255, 0] == 4096 and got[0, min(sa, 255)] == -4096


def test_apply_rules():
    rec = np.zeros((6, 24), np.float32)
    rec[:, 4:8] = (0.5, 0.25, 0.75, 0.6)
    rec[5, 5] = np.nan
    one = 65536
    num = np.array([[-one * 2048] * 3, [one * 4096] * 3, [-one * 4096] * 3, [one * 100] * 3, [one * 100] * 3, [one * 1024] * 3], np.int64)
    den = np.array([one, one, one, one - 1, 0, one], np.uint64)
    out, counts = rr.apply(rec, num, den, 0.5, 1.0)
    assert out[0, 4:7].tolist() == [0.25, 0.0, 0.5]                             # -0.5 * 0.5; green lands on 0 exactly: not clamped
    assert out[1, 4:7].tolist() == [1.0, 0.75, 1.0]                             # +1 * 0.5; blue clamps at 1
    assert out[2, 4:7].tolist() == [0.0, 0.0, 0.25]
    assert np.array_equal(out[3:5].view(np.uint32), rec[3:5].view(np.uint32))   # below the threshold, and den = 0
    assert out[5, 4] == np.float32(0.625) and np.isnan(out[5, 5]) and out[5, 6] == np.float32(0.875)
    assert counts == dict(records=6, updated=4, clamped=2, no_weight=2)
    assert np.array_equal(out[:, 7], rec[:, 7])
    assert rr.threshold(0.0) == 0 and rr.threshold(1.0) == 65536 and rr.threshold(3e38) == (1 << 64) - 1


def overlapping_opaque_quads(W, H):
    """Opaque Gaussians on a 4-pixel lattice, each 16 pixels wide: every pixel of the frame saturates under several."""
    qs = [sr.quad_at(W, H, x, y, 8.0, rgb=(0.5, 0.5, 0.5), a=1.0, conic=(0.03, 0.0, 0.03)) for y in range(2, H, 4) for x in range(2, W, 4)]
    return np.stack(qs)


def albedo_sse(target, render):
    both = (target[..., 3] != 0) & (render[..., 3] != 0)
    d = target[..., :3].astype(np.int64) - render[..., :3].astype(np.int64)
    return int((d * d)[both].sum())


def test_one_step_removes_a_uniform_colour_error():
    """The property tests/test_gpu_refit.py's end-to-end case rests on, by the restatement alone: uniform colour 0.5 under a constant
    target (204, 102, 51); one iteration at step 1 leaves a few LSB of 76, so the SSE falls far below a quarter."""
    W, H = 64, 32
    q = overlapping_opaque_quads(W, H)
    n = q.shape[0]
    target = np.zeros((H, W, 4), np.uint8)
    target[:] = (204, 102, 51, 255)
    s = sr.setup(q, W, H)
    render = sr.render(q, W, H, 0, s=s)[0][2]
    assert render[..., 3].min() >= 250
    before = albedo_sse(target, render)
    ref = rr.accumulate(q, np.arange(n), n, W, H, target, render, 128, s=s)
    assert ref["pixels"] == W * H and (ref["den"] > 0).all()
    rec = np.zeros((n, 24), np.float32)
    rec[:, 4:8] = q[:, 8:12]
    out, counts = rr.apply(rec, ref["num"], ref["den"], 1.0, 1.0)
    assert counts["updated"] > n // 2
    q2 = q.copy()
    q2[:, 8:11] = out[:, 4:7]
    after = albedo_sse(target, sr.render(q2, W, H, 0, s=sr.setup(q2, W, H))[0][2])
    print(f"albedo SSE {before} -> {after} ({after / before:.5f})")
    assert before > W * H * 50 * 50 and after * 4 < before


def test_struct_sizes():
    from mesh2splat_amd import refit
    assert C.sizeof(refit.RefitParamsC) == 16 and C.sizeof(refit.RefitApplyParamsC) == 16
