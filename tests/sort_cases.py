"""Shared inputs of the depth-sort tests (test_sort_cases_cpu.py proves them, test_gpu_sort_ranges.py runs them): records whose depth
keys are crafted bit patterns, and the one reference every comparison uses — numpy float32 in the key kernel's association, then a stable
argsort on the raw bits.  numpy only.

m2s_sort.hip chooses its sort from the keys it has just built: `key - min` over the bits that differ when the range fits 24 bits
("reduced"), SubtractOrBehind over up to 32 bits when the frustum test is applied by the sort ("cull"), else all 32 bits ("plain").
Below that choice the library picks an algorithm from n (one block / merge sort / onesweep).  The sets here are named after the key
range they produce, so that every branch, and every edge between two branches, has a set that is known to take it."""
import numpy as np

f32 = np.float32

# every size at which something changes: one record, a wave (64) and the key kernels' workgroup (256) minus / plus one, the library's
# one-block sort (<= 1024), and a merge-sort size of many workgroups that is no multiple of 64 x anything
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 40_000)
CULL_SIZES = (1, 64, 65, 1025, 40_000)


def down_and_up(sizes):
    """The sizes in an order that goes down and comes up again (largest first, the second largest last): grow-only buffers, the work
    area's tail and the position plane meet a large n, small ones, and a large one again."""
    s = sorted(sizes, reverse=True)
    return s[0::2] + s[1::2][::-1]


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def depth_view(scale: float = 1.0, shift: float = 0.0, axis: int = 0) -> np.ndarray:
    """World-to-view matrix (applied as M @ (P, 1)) whose depth row is (scale, 0, 0, shift): view-space z = scale * x + shift (axis 1, 2:
    y, z in place of x)."""
    v = np.eye(4, dtype=f32)
    v[2] = (0.0, 0.0, 0.0, shift)
    v[2, axis] = scale
    return v


def want_keys(rec: np.ndarray, view: np.ndarray) -> np.ndarray:
    """uint32[n]: the raw bits of view-space z, ((v02*x + v12*y) + v22*z) + v32 in float32 — k_depth_keys' association."""
    with np.errstate(all="ignore"):
        z = (f32(view[2, 0]) * rec[:, 0] + f32(view[2, 1]) * rec[:, 1]) + f32(view[2, 2]) * rec[:, 2]
        z = (z + f32(view[2, 3])).astype(f32)
    return z.view(np.uint32)


def want_order(keys: np.ndarray) -> np.ndarray:
    return np.argsort(keys, kind="stable")


def want_sorted(rec: np.ndarray, view: np.ndarray) -> np.ndarray:
    """The records in depth order: ascending on the raw key bits, equal keys in input order."""
    return rec[want_order(want_keys(rec, view))]


# ---- records ----------------------------------------------------------------------------------------------------------------------------
def _distinct_words(count: int, seed: int) -> np.ndarray:
    """`count` distinct pseudo-random uint32: a bijection of 0 .. count-1 (odd multiplier, then two xor-shifts)."""
    v = np.arange(count, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed & 0xFFFFFFFF)
    v &= np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(13)
    return v.astype(np.uint32)


INDEX_WORD = 23          # the word of records_with_keys' records that holds the record's index


def records_with_keys(bits, seed: int = 0) -> np.ndarray:
    """(n, 24) float32 records at (x, 0, 0), x having exactly the uint32 bit pattern bits[i].  Word 23 is the record's index; the other
    twenty words are distinct random bit patterns (no two equal anywhere in the array), so that a gather that mixes quads or rows shows."""
    bits = np.ascontiguousarray(bits, np.uint32).reshape(-1)
    n = bits.shape[0]
    w = np.zeros((n, 24), np.uint32)
    fill = [c for c in range(3, 24) if c != INDEX_WORD]
    w[:, fill] = _distinct_words(n * len(fill), seed).reshape(n, len(fill))
    w[:, INDEX_WORD] = np.arange(n, dtype=np.uint32)
    w[:, 0] = bits
    return w.view(f32)


# ---- key sets for m2s_sort_by_depth -----------------------------------------------------------------------------------------------------
MIN_LO, MIN_HI = 0x00000001, 0xC0800000          # the smallest positive denormal; -4.0 (keys up to -16.0: no NaN pattern in reach)
RANGES = (0x0, 0x1, 0xFF, 0x100, 0xFFFF, 0x10000, 0xFFFFFF, 0x1000000)
# name -> (range, smallest key): range_<hex>_lo on the small minimum, range_<hex>_hi on the large one
RANGE_SETS = {f"range_{r:x}_{tag}": (r, m) for r in RANGES for tag, m in (("lo", MIN_LO), ("hi", MIN_HI))}
SPECIAL_SETS = ("mixed_sign", "denormals", "quiet_nans")
KEY_SETS = tuple(RANGE_SETS) + SPECIAL_SETS

QNAN_POS, QNAN_NEG = 0x7FC00000, 0xFFC00000
INF_POS, INF_NEG = 0x7F800000, 0xFF800000
_MIXED = (0x80000000, 0x00000000,                # -0, +0 (the key kernel's additions turn -0 into +0: the reference does the same)
          INF_NEG, INF_POS, 0x7F7FFFFF, 0xFF7FFFFF,          # both infinities, the largest finite values
          0x00000001, 0x80000001, 0x00800000, 0x80800000)    # the smallest denormals and the smallest normal values


def _tiled(pattern: np.ndarray, n: int) -> np.ndarray:
    """The pattern repeated up to n entries: entry i equals entry i + len(pattern) — equal keys at non-adjacent positions from n = 3 on
    (every pattern here has at least two entries)."""
    return np.tile(pattern, n // pattern.shape[0] + 1)[:n]


def _half(n: int) -> int:
    return max(2, (n + 1) // 2)


def _range_offsets(r: int, n: int, rng) -> np.ndarray:
    """n offsets in [0, r], both ends present (n >= 2), every value at least twice (n >= 3; an odd n leaves one value single)."""
    if n == 1:
        return np.zeros(1, np.uint64)
    p = rng.integers(0, r + 1, _half(n), dtype=np.uint64)
    p[0], p[-1] = r, 0
    return _tiled(p, n)


def _finite_bits(count: int, rng, exp_lo: int = 1, exp_hi: int = 254) -> np.ndarray:
    """random finite float32 bit patterns of both signs with a biased exponent in [exp_lo, exp_hi]"""
    sign = rng.integers(0, 2, count, dtype=np.uint64) << np.uint64(31)
    expo = rng.integers(exp_lo, exp_hi + 1, count, dtype=np.uint64) << np.uint64(23)
    return (sign | expo | rng.integers(0, 1 << 23, count, dtype=np.uint64)).astype(np.uint32)


def _with_specials(specials, rest: np.ndarray, n: int) -> np.ndarray:
    p = np.concatenate([np.asarray(specials, np.uint32), rest])[:_half(n)]
    return _tiled(p, n)


def key_bits(name: str, n: int) -> np.ndarray:
    """uint32[n]: the x bit patterns of the named set at size n (deterministic)."""
    rng = np.random.default_rng([KEY_SETS.index(name), n])
    if name in RANGE_SETS:
        r, m = RANGE_SETS[name]
        return (np.uint64(m) + _range_offsets(r, n, rng)).astype(np.uint32)
    h = _half(n)
    if name == "mixed_sign":        # in front of and behind the camera, with every special value: a range of 2^31 and more from n = 63 on
        return _with_specials(_MIXED, _finite_bits(h, rng), n)
    if name == "denormals":         # exponent field 0 throughout, both signs
        rest = (rng.integers(0, 2, h, dtype=np.uint64) << np.uint64(31)) | rng.integers(1, 1 << 23, h, dtype=np.uint64)
        return _with_specials((0x00000001, 0x807FFFFF, 0x007FFFFF, 0x80000001), rest.astype(np.uint32), n)
    if name == "quiet_nans":        # the two quiet NaNs and their signs' infinities among finite keys of ordinary size
        return _with_specials((QNAN_POS, QNAN_NEG, INF_POS, INF_NEG), _finite_bits(h, rng, 100, 150), n)
    raise KeyError(name)


def second_view() -> np.ndarray:
    """The view of every case's second sort (its keys come from the position plane the first sort left behind): the same row scaled by
    2, shifted by 0.  Doubling adds one to the exponent field — the keys of a *_hi range set move by 0x00800000 and keep their range
    exactly, infinities, NaNs, zeros and signs stay what they are, denormals stay denormal or become the smallest normal values — and 0
    is the only shift that keeps a crafted bit pattern: any other constant rounds the low bits of most keys away.  (The *_lo sets
    start at a denormal, whose bits double instead: their second sort has another range, and is checked against the reference all the
    same.)"""
    return depth_view(2.0, 0.0)


# ---- sets for m2s_prepass_sorted without a depth image (the sort applies the frustum test: "cull mode") ---------------------------------
Z_FIRST = 0xBF800000                                       # -1.0: the survivors' smallest key
Z_NEAR, Z_FAR = 0xBCA3D70A, 0xC2B40000                     # -0.02 and -90.0: the wide set's ends
CULLED_X = f32(1e6)
# name -> (range of the survivors' keys, smallest survivor key, layout)
#   "one": one survivor, in the middle of the culled        "thirds": every third record culled — both kinds in every wave
#   "waves": whole waves culled, every other one             "none" / "all": nothing / everything culled
CULL_SETS = {
    "cull_one_survivor": (0x0, Z_FIRST, "one"),
    "cull_range_1": (0x1, Z_FIRST, "thirds"),
    "cull_range_fffffe": (0xFFFFFE, Z_FIRST, "thirds"),     # `behind` = range + 1 = 0xFFFFFF: 24 bits
    "cull_range_ffffff": (0xFFFFFF, Z_FIRST, "thirds"),     # `behind` = 0x1000000: 25 bits
    "cull_wide": (Z_FAR - Z_NEAR, Z_NEAR, "thirds"),
    "cull_whole_waves": (Z_FAR - Z_NEAR, Z_NEAR, "waves"),
    "cull_none": (0xFFFFFF, Z_FIRST, "none"),
    "cull_all": (0x0, Z_FIRST, "all"),
}


def cull_survivors(name: str, n: int) -> np.ndarray:
    """bool[n]: which records of the set are placed inside the frustum"""
    i = np.arange(n)
    layout = CULL_SETS[name][2]
    if layout == "one":
        return i == n // 2
    if layout == "thirds":
        return i % 3 != 1
    if layout == "waves":
        return (i // 64) % 2 == 1
    return np.full(n, layout == "none")


def cull_records(name: str, n: int) -> np.ndarray:
    """(n, 24) float32 records of the named cull set: survivors at (0, 0, z) with crafted z bits, culled records at x = 1e6 with z drawn
    from the survivors' interval (a culled record that were sorted as a survivor would land among them).  The other fields are those of
    an ordinary opaque Gaussian — three scales of 1 to 10 % of the depth, so that every splat is an ellipse of 8 to 80 pixels (a circle,
    which a sphere seen head-on or anything smaller than the 0.3-pixel low-pass becomes, makes the shader's quad axes 0 / 0 = NaN), unit
    quaternion, unit normal — and word 20 (pbr.x, which the prepass copies into the
    quad) is the record's index."""
    r, zmin, _ = CULL_SETS[name]
    rng = np.random.default_rng([len(KEY_SETS) + list(CULL_SETS).index(name), n])
    alive = cull_survivors(name, n)
    m = int(alive.sum())
    z = (np.uint64(zmin) + rng.integers(0, r + 1, n, dtype=np.uint64)).astype(np.uint32)
    if m:
        z[alive] = (np.uint64(zmin) + _range_offsets(r, m, rng)).astype(np.uint32)
    rec = np.zeros((n, 24), f32)
    rec[:, 0] = np.where(alive, f32(0), CULLED_X)
    rec[:, 2] = z.view(f32)
    rec[:, 3] = 1
    rec[:, 4:7] = rng.uniform(0, 1, (n, 3))
    rec[:, 7] = 1
    rec[:, 8:11] = np.abs(rec[:, 2:3]) * np.exp(rng.uniform(np.log(0.01), np.log(0.1), (n, 3)))
    v = rng.normal(size=(n, 3))
    rec[:, 12:15] = v / np.linalg.norm(v, axis=1, keepdims=True)
    q = rng.normal(size=(n, 4))
    rec[:, 16:20] = q / np.linalg.norm(q, axis=1, keepdims=True)
    rec[:, 20] = np.arange(n)
    rec[:, 21] = rng.uniform(0, 1, n)
    rec[:, 23] = 1
    return rec


def m4_mul(m: np.ndarray, p: np.ndarray) -> np.ndarray:
    """mat4 * vec4 in float32 with the shader's association, (m0*x + m1*y) + (m2*z + m3*w); m in glm's memory order (m[c] = column c),
    p (n, 4)"""
    m = np.asarray(m, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        cols = [(m[0, i] * p[:, 0] + m[1, i] * p[:, 1]) + (m[2, i] * p[:, 2] + m[3, i] * p[:, 3]) for i in range(4)]
    return np.stack(cols, 1).astype(f32)


def frustum_test(rec: np.ndarray, model, view, proj):
    """The prepass's first lines (gaussianSplattingPrepassCS.glsl:67-77) in float32 -> (inside bool[n], view-space z bits uint32[n])."""
    one = np.ones((rec.shape[0], 1), f32)
    ws = m4_mul(model, np.concatenate([rec[:, 0:3], one], 1))
    vs = m4_mul(view, np.concatenate([ws[:, 0:3], one], 1))
    c = m4_mul(proj, vs)
    clip = f32(1.05) * c[:, 3]
    with np.errstate(all="ignore"):
        outside = (c[:, 2] < -clip) | (c[:, 0] < -clip) | (c[:, 0] > clip) | (c[:, 1] < -clip) | (c[:, 1] > clip)
    return ~outside, np.ascontiguousarray(vs[:, 2]).view(np.uint32)
