"""Numpy restatement of m2s_score_frames (include/m2s.h: the pin).  Plain int64 and float64, one 8 x 8 window at a time from the
pixels themselves — no cells, no tiles, nothing shared with the kernel's decomposition.  Images are (H, W, 4) uint8 arrays, row 0 = the
bottom row (the orientation does not matter to any figure; the window origins count from row 0 / column 0)."""
import numpy as np

C1, C2 = 26634, 239708            # (0.01 * 255)^2 * 64^2 and (0.03 * 255)^2 * 64^2, truncated
NO_COVER, WANT_MAP = 1, 2


def luma(img):
    p = img.astype(np.int64)
    return (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8


def mask_of(mode, in_a, in_b):
    return {0: np.ones_like(in_a), 1: in_a, 2: in_a | in_b, 3: in_a & in_b}[mode]


def window_q(ya, yb):
    """q = llrint(ssim * 2^32) of one window from its two 8 x 8 luma blocks (int64)."""
    s1, s2 = int(ya.sum()), int(yb.sum())
    ssq = int((ya * ya).sum() + (yb * yb).sum())
    s12 = int((ya * yb).sum())
    num = (2 * s1 * s2 + C1) * (128 * s12 - 2 * s1 * s2 + C2)
    den = (s1 * s1 + s2 * s2 + C1) * (64 * ssq - s1 * s1 - s2 * s2 + C2)
    assert abs(num) < 2 ** 59 and 0 < den < 2 ** 59
    ssim = np.float64(np.int64(num)) / np.float64(np.int64(den))      # both conversions and the division correctly rounded
    return int(np.rint(ssim * np.float64(4294967296.0))), (s1, s2, ssq, s12)


def score(a, b, cover_a=None, cover_b=None, mask_mode=0, flags=0):
    """-> dict with the fields of m2s_score_result (python ints / lists) and "map" ((H, W, 4) uint8, or None without WANT_MAP)."""
    H, W = a.shape[:2]
    assert a.shape == b.shape == (H, W, 4) and a.dtype == b.dtype == np.uint8
    if flags & NO_COVER:
        in_a = in_b = np.ones((H, W), bool)
    else:
        in_a, in_b = cover_a[..., 3] != 0, cover_b[..., 3] != 0
    m = mask_of(mask_mode, in_a, in_b)
    d = np.abs(a[..., :3].astype(np.int64) - b[..., :3].astype(np.int64))
    dm = d[m]
    out = {"pixels": int(m.sum()),
           "cover": [int((~in_a & ~in_b).sum()), int((in_a & ~in_b).sum()), int((~in_a & in_b).sum()), int((in_a & in_b).sum())],
           "sse": [int((dm[:, c] * dm[:, c]).sum()) for c in range(3)], "sad": [int(dm[:, c].sum()) for c in range(3)],
           "max_abs": [int(dm[:, c].max()) if len(dm) else 0 for c in range(3)]}
    ya, yb = luma(a), luma(b)
    windows, total = 0, 0
    for y in range(0, H - 7, 4):
        for x in range(0, W - 7, 4):
            if int(m[y:y + 8, x:x + 8].sum()) < 32:
                continue
            q, _ = window_q(ya[y:y + 8, x:x + 8], yb[y:y + 8, x:x + 8])
            windows += 1
            total += q
    out["windows"], out["ssim_q32"] = windows, total
    out["map"] = None
    if flags & WANT_MAP:
        mp = np.zeros((H, W, 4), np.uint8)
        mp[..., :3] = np.where(m[..., None], d, 0)
        mp[..., 3] = np.where(m, 255, 0)
        out["map"] = mp
    return out


FIELDS = ("pixels", "cover", "sse", "sad", "max_abs", "windows", "ssim_q32")


def psnr(r):
    if r["pixels"] == 0:
        return float("nan")
    sse = sum(r["sse"])
    return float("inf") if sse == 0 else float(10.0 * np.log10(65025.0 * 3.0 * r["pixels"] / sse))
