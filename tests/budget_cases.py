"""Shared inputs of the budget tests: the key families (crafted accumulators) and the planted AREA records."""
import numpy as np

SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4099)      # round the wave and workgroup edges; more than one workgroup per histogram
FAMILIES = ("random", "all_equal", "digit0", "digit1", "digit2", "digit3", "half_zero")
ONE = 0x3F800000


def budgets(n):
    return sorted({max(1, b) for b in (1, n // 2, n - 1, n, n + 5)})


def family(name, n, seed=0):
    """-> (wmax bits uint32[n], npix uint32[n]).
    random:    wmax bits anywhere in [0, bits(1.0)] (denormals included), npix in 0..50
    all_equal: one key: the selection is all ties and keeps the first B by index
    digit0..2: npix = 1 and wmax bits 0x3F000000 | (v << 8k): the keys differ in ONE byte, so only the round of that byte decides
               (k = 2: v < 0x80, so that the weight stays below 1)
    digit3:    npix = 1, the top byte from {0x00, 0x10, 0x20, 0x3F} over zeros: the first round decides, the rest see ties
    half_zero: random with half the keys zero (npix = 0)"""
    rng = np.random.default_rng(1000 * FAMILIES.index(name) + seed + n)
    if name in ("random", "half_zero"):
        w = rng.integers(0, ONE + 1, n, dtype=np.uint32)
        k = rng.integers(0, 51, n, dtype=np.uint32)
        if name == "half_zero":
            k[rng.random(n) < 0.5] = 0
        return w, k
    if name == "all_equal":
        return np.full(n, 0x3F000000, np.uint32), np.full(n, 7, np.uint32)
    one = np.ones(n, np.uint32)
    if name == "digit3":
        return (rng.choice(np.array([0x00, 0x10, 0x20, 0x3F], np.uint32), n) << np.uint32(24)).astype(np.uint32), one
    k = int(name[-1])
    v = rng.integers(0, 0x80 if k == 2 else 0x100, n, dtype=np.uint32)
    return (np.uint32(0x3F000000) | (v << np.uint32(8 * k))).astype(np.uint32), one


def records(n, seed=0):
    """n tame records, every word distinct enough that a misplaced row shows."""
    rng = np.random.default_rng(seed)
    rec = rng.normal(0, 1, (n, 24)).astype(np.float32)
    rec[:, 7] = rng.random(n)                            # alpha
    rec[:, 8:10] = np.exp(rng.normal(-1, 1, (n, 2)))     # scale
    return rec


def planted_area_records(n=300, seed=5):
    """records() with what a .ply can hold planted in the fields the AREA key reads."""
    rec = records(n, seed)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    rec[3, 8] = nan                                      # NaN scale -> key 0
    rec[10, 9] = nan
    rec[20, 8] = -2.5                                    # negative scale: its magnitude counts
    rec[21, 8:10] = (-3.0, -4.0)
    rec[30, 8], rec[30, 7] = inf, 0.0                    # inf * 0 = NaN -> key 0
    rec[40, 8], rec[40, 7] = inf, 1.0                    # +inf: the largest key
    rec[41, 9], rec[41, 7] = -inf, 0.5                   # (also +inf)
    rec[50, 7] = 7.0                                     # alpha above 1 -> 1
    rec[51, 7] = -0.25                                   # alpha below 0 -> 0 -> key 0
    rec[52, 7] = -0.0
    rec[60, 7] = nan                                     # alpha NaN -> 0 -> key 0
    rec[61, 7], rec[61, 8] = nan, inf                    # 0 * inf -> key 0
    rec[70, 8] = 0.0
    rec[71, 8] = -0.0
    rec[80, 8:10] = (1e-30, 1e-30)                       # the product underflows to 0
    rec[81, 8:10] = (1e-20, 1e-22)                       # a denormal product
    rec[90, 8:10] = (1e30, 1e30)                         # the product overflows to +inf
    return rec
